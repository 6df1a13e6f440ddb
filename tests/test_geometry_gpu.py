"""GPU: the input geometry (mi355enc_set_input_geometry / mi355enc_set_crop, k_scale.hip's GEOM form) -- the launch bit-exact
against tests/geomref.py, nothing outside the crop rectangle reaching the output, the degenerate geometry equal to the scaler, streams equal to those of a plain
encoder fed geomref's pictures (so every coded source is geomref's), and the crop changing while pictures are in flight."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import geomref as G
from tests import orientref, overlayref, spsref

pytestmark = pytest.mark.gpu

FMTS = [G.FMT_NV12, G.FMT_I420, G.FMT_YUY2, G.FMT_UYVY]
FMT_IDS = ["nv12", "i420", "yuy2", "uyvy"]
JPEG = os.path.join(os.path.dirname(__file__), "golden", "jpeg", "q50_420_72x40.jpg")
GOP, QP, N = 30, 28, 5

# (input size, crop, destination, target): tiles are 64 bytes x 16 rows
CASES = {
    "down-off-grid": ((160, 96), (18, 10, 120, 70), (22, 6, 100, 36), (144, 48)),      # one tile wholly border, several straddle
    "up-2.5": ((160, 96), (40, 20, 40, 24), (10, 4, 100, 60), (144, 80)),              # 4:2:2 chroma rows at s = 0.4 < 1/2
    "mixed": ((160, 96), (0, 2, 160, 24), (4, 2, 80, 60), (100, 64)),                  # down 2 across, up 2.5 down the picture
    "s8": ((144, 132), (2, 2, 128, 128), (8, 8, 16, 16), (32, 32)),
    "s1/8": ((32, 24), (4, 4, 16, 16), (2, 0, 128, 128), (132, 128)),
    "422-quarter": ((64, 32), (6, 8, 40, 16), (0, 2, 40, 64), (48, 66)),               # chroma-row stretch max(2 s, 1) = 1 at s = 1/4
    "far-edge": ((160, 96), (100, 60, 60, 36), (0, 0, 144, 48), (144, 48)),            # the crop touches the picture's far edge
}


def planes_of(fmt, w, h, rng, pad=0, offset=0, saturated=False):
    """planes of a w x h picture in `fmt`: seeded noise, or a 0 / 255 checkerboard; pad: extra bytes per row, offset: the first sample's offset in its buffer"""
    def mk(rows, cols):
        buf = rng.integers(0, 256, rows * (cols + pad) + offset, dtype=np.uint8)
        v = np.lib.stride_tricks.as_strided(buf[offset:], (rows, cols), (cols + pad, 1))
        if saturated:
            v[:] = (((np.arange(rows)[:, None] // 3 + np.arange(cols)[None, :] // 5) & 1) * 255).astype(np.uint8)
        return v
    if fmt == G.FMT_NV12:
        return [mk(h, w), mk(h // 2, w)]
    if fmt == G.FMT_I420:
        return [mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2)]
    return [mk(h, 2 * w)]


def encoder(E, case, border=G.BLACK, keep_sar=False, **kw):
    insize, crop, dst, (tw, th) = case
    return E.Encoder(tw, th, fixed_qp=QP, gop=GOP, geometry=E.geometry(insize, crop=crop, dst=dst, border=border, keep_sar=keep_sar), **kw)


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_stage_geometry_is_bit_exact(E, fmt, name):
    insize, crop, dst, (tw, th) = CASES[name]
    border = (37, 201, 90)
    e = encoder(E, CASES[name], border=border)
    for k, sat in enumerate((False, False, True)):
        pl = planes_of(fmt, insize[0], insize[1], np.random.default_rng(1000 * fmt + k), pad=3 * k, offset=k, saturated=sat)
        dy, duv = e.stage_geometry(fmt, pl)
        ry, ruv = G.to_nv12(fmt, pl, insize[0], insize[1], crop, dst, tw, th, border)
        assert np.array_equal(dy, ry), (k, np.argwhere(dy != ry)[:4])
        assert np.array_equal(duv, ruv), (k, np.argwhere(duv != ruv)[:4])
    e.close()


def test_default_border_is_black_and_stage_scale_keeps_its_contract(E):
    case = CASES["down-off-grid"]
    e = encoder(E, case)
    pl = planes_of(G.FMT_NV12, 160, 96, np.random.default_rng(5))
    dy, duv = e.stage_geometry(G.FMT_NV12, pl)
    ry, ruv = G.to_nv12(G.FMT_NV12, pl, 160, 96, case[1], case[2], 144, 48)
    assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
    assert dy[0, 0] == 16 and tuple(duv[0, 0:2]) == (128, 128)
    e.close()
    p = E.Encoder(144, 48, fixed_qp=QP)  # without a geometry: the new entry point refuses, the old one still refuses upscaling
    with pytest.raises(E.EncoderError):
        p.stage_geometry(G.FMT_NV12, pl)
    with pytest.raises(E.EncoderError):
        p.set_input_size(72, 24)
    p.close()


def _outside_replaced(fmt, pl, w, h, crop, rng, pad=0, offset=0):
    """a copy of the planes whose every sample outside the crop rectangle is new noise (4:2:0 chroma: outside the crop's chroma rectangle); pad, offset: each
    plane lies in a noise container with `pad` more bytes per row than it shows, from byte `offset` on"""
    cx, cy, cw, ch = crop
    out = []
    for i, p in enumerate(pl):
        rows, cols = p.shape
        buf = rng.integers(0, 256, rows * (cols + pad) + offset, dtype=np.uint8)
        q = np.lib.stride_tricks.as_strided(buf[offset:], (rows, cols), (cols + pad, 1))
        if fmt in (G.FMT_YUY2, G.FMT_UYVY):
            q[cy:cy + ch, 2 * cx:2 * (cx + cw)] = p[cy:cy + ch, 2 * cx:2 * (cx + cw)]
        elif i == 0:
            q[cy:cy + ch, cx:cx + cw] = p[cy:cy + ch, cx:cx + cw]
        elif fmt == G.FMT_NV12:
            q[cy // 2:(cy + ch) // 2, cx:cx + cw] = p[cy // 2:(cy + ch) // 2, cx:cx + cw]
        else:
            q[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2] = p[cy // 2:(cy + ch) // 2, cx // 2:(cx + cw) // 2]
        out.append(q)
    return out


@pytest.mark.parametrize("name", ["down-off-grid", "up-2.5", "far-edge"])
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_nothing_outside_the_crop_reaches_the_output(E, fmt, name):
    insize, crop, dst, (tw, th) = CASES[name]
    e = encoder(E, CASES[name])
    rng = np.random.default_rng(77 + fmt)
    pl = planes_of(fmt, insize[0], insize[1], rng)
    ref = G.to_nv12(fmt, pl, insize[0], insize[1], crop, dst, tw, th)
    for k in range(2):
        other = _outside_replaced(fmt, pl, insize[0], insize[1], crop, rng, pad=5 + 2 * k, offset=1 + k)  # (noise beyond the visible width too)
        assert not np.array_equal(other[0], pl[0])
        dy, duv = e.stage_geometry(fmt, other)
        assert np.array_equal(dy, ref[0]) and np.array_equal(duv, ref[1]), k
    e.close()


# ---- streams
def run(e, feed, n, depth=2, before=None):
    out = []
    for i in range(n):
        if before:
            before(i)
        feed(i)
        if e.pending > depth:
            out.append(e.collect())
    while e.pending:
        out.append(e.collect())
    return out, (e.fetch(0), e.fetch(1))


def plain_stream(E, w, h, pictures, setup=None, **kw):
    """the stream of a plain encoder fed finished w x h pictures"""
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, **kw)
    if setup:
        setup(e)
    res = run(e, lambda i: e.submit(pictures[i][0], pictures[i][1], pts=i), len(pictures))
    e.close()
    return res


def same(got, ref):
    (ga, grec), (ra, rrec) = got, ref
    assert len(ga) == len(ra)
    for i, (g, r) in enumerate(zip(ga, ra)):
        assert g == r, (i, len(g[0]), len(r[0]), g[1:], r[1:])
    assert np.array_equal(grec[0], rrec[0]) and np.array_equal(grec[1], rrec[1])


def nv12_clip(w, h, n, seed):
    """n NV12 pictures: noise, then drifting copies with fresh noise mixed in (P pictures with work to do)"""
    base = orientref.noise(w, h, seed)
    pics = []
    for i in range(n):
        fresh = orientref.noise(w, h, seed + 1 + i)
        y = np.where(fresh[0] < 40, fresh[0], np.roll(base[0], 2 * i, axis=1))
        uv = np.where(fresh[1] % 8 == 0, fresh[1], np.roll(base[1], 2 * i, axis=1))
        pics.append((np.ascontiguousarray(y), np.ascontiguousarray(uv)))
    return pics


def geom_pictures(pics, insize, crop, dst, tw, th, border=G.BLACK):
    """geomref's visible tw x th NV12 picture of every input picture; crop: one rectangle, or one per picture"""
    out = []
    for i, (y, uv) in enumerate(pics):
        c = crop[i] if isinstance(crop, list) else crop
        sy, suv = G.to_nv12(G.FMT_NV12, [y, uv], insize[0], insize[1], c, dst, tw, th, border)
        out.append((np.ascontiguousarray(sy[:th, :tw]), np.ascontiguousarray(suv[:th // 2, :tw])))
    return out


def test_degenerate_geometry_is_the_scaler(E):
    iw, ih, w, h = 192, 112, 96, 56
    pics = nv12_clip(iw, ih, N, 300)
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, input_size=(iw, ih))
    ref = run(a, lambda i: a.submit(*pics[i], pts=i), N)
    a.close()
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((iw, ih), target=(w, h)))
    got = run(b, lambda i: b.submit(*pics[i], pts=i), N)
    sy, suv = b.stage_geometry(G.FMT_NV12, list(pics[0]))
    b.close()
    same(got, ref)
    c = E.Encoder(w, h, fixed_qp=QP, input_size=(iw, ih))
    cy, cuv = c.stage_scale(G.FMT_NV12, list(pics[0]))
    c.close()
    assert np.array_equal(sy, cy) and np.array_equal(suv, cuv)


def _sse(src, dec, w, h):
    (sy, suv), (dy, duv) = src, dec
    d = lambda a, b: int(((a.astype(np.int64) - b.astype(np.int64)) ** 2).sum())
    return (d(sy[:h, :w], dy[:h, :w]), d(suv[:h // 2, 0:w:2], duv[:h // 2, 0:w:2]), d(suv[:h // 2, 1:w:2], duv[:h // 2, 1:w:2]))


@pytest.mark.parametrize("method", [0, 1], ids=["identity", "90r-overlay"])
def test_pillarbox_stream(E, oracle, method):
    """a portrait 48 x 80 picture pillarboxed into a 96 x 64 programme; with 90r the programme is 64 x 96, the geometry's target stays 96 x 64, and a text
    is drawn on the turned picture"""
    iw, ih, tw, th = 48, 80, 96, 64
    dst = E.fit_rect(iw, ih, tw, th)
    assert dst == G.fit_rect(iw, ih, tw, th) == (28, 0, 38, 64)
    crop = (0, 0, iw, ih)
    pics = nv12_clip(iw, ih, N, 400)
    want = geom_pictures(pics, (iw, ih), crop, dst, tw, th)
    w, h = orientref.size(method, tw, th)
    if method:
        want = [orientref.orient(y, uv, method) for y, uv in want]
    text = "12:34" if method else None
    setup = (lambda enc: enc.set_overlay_text(text)) if text else None
    ref = plain_stream(E, w, h, want, setup=setup)
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=2, orientation=method or None,
                  geometry=E.geometry((iw, ih), crop=crop, dst=dst, keep_sar=True))
    if setup:
        setup(e)
        want = [overlayref.draw(y, uv, text) for y, uv in want]  # (the coded source carries the text)
    e.set_quality_metrics(True)
    out, dec, sse = [], oracle.Decoder(), []
    for i in range(N):
        e.submit(*pics[i], pts=i)
        if e.pending > 2:
            out.append(e.collect())
            sse.append(tuple(e.last_quality().sse))
    while e.pending:
        out.append(e.collect())
        sse.append(tuple(e.last_quality().sse))
    got = (out, (e.fetch(0), e.fetch(1)))
    e.close()
    same(got, ref)
    assert spsref.sps_of(out[0][0])[0]["sar"] is None  # KEEP_SAR: the headers of an unscaled stream
    # picture by picture, without a pipeline: the same access units, reconstruction == decode, and the metrics' reference surface -- the coded source -- is
    # geomref's picture (turned by orientref, the text drawn by overlayref)
    one = E.Encoder(w, h, gop=GOP, fixed_qp=QP, orientation=method or None, geometry=E.geometry((iw, ih), crop=crop, dst=dst, keep_sar=True))
    if setup:
        setup(one)
    for i, au in enumerate(out):
        assert one.encode(*pics[i], pts=i)[0] == au[0], i
        dy, duv = dec.decode(au[0])
        assert np.array_equal(dy, one.fetch(0)) and np.array_equal(duv, one.fetch(1)), i
        assert sse[i] == _sse(want[i], (dy, duv), w, h), i
    one.close()
    assert np.array_equal(dy, got[1][0]) and np.array_equal(duv, got[1][1])
    if not method:  # the border columns of the coded source are the border colour, so the decoded ones are near it
        assert abs(int(dy[:th, :dst[0]].astype(np.int64).mean()) - 16) <= 3


def test_exact_sar_in_the_sps_and_exchanged_when_turned(E):
    iw, ih, tw, th = 160, 96, 144, 48
    crop, dst = (18, 10, 120, 70), (22, 6, 100, 36)
    pics = nv12_clip(iw, ih, 1, 500)
    for method in (0, 1):
        w, h = orientref.size(method, tw, th)
        e = E.Encoder(w, h, fixed_qp=QP, orientation=method or None, geometry=E.geometry((iw, ih), crop=crop, dst=dst))
        au = e.encode(*pics[0])[0]
        e.close()
        assert spsref.sps_of(au)[0]["sar"] == G.sar(crop, dst, transposed=bool(method))


def test_either_order_with_the_orientation_and_with_the_input_size(E):
    iw, ih, tw, th = 48, 80, 96, 64
    g = E.geometry((iw, ih), dst=(28, 0, 38, 64), keep_sar=True)
    pics = nv12_clip(iw, ih, 2, 600)
    streams = []
    for order in (0, 1):
        e = E.Encoder(th, tw, fixed_qp=QP, gop=GOP)  # the programme is 64 x 96: turned
        if order == 0:
            with pytest.raises(E.EncoderError):  # (against the unturned 64 x 96 target the destination rectangle does not fit: refused, the handle as it was)
                e.set_input_geometry(g)
            e.set_orientation("90r")
            e.set_input_geometry(g)
        else:
            e.set_orientation("90r")
            e.set_input_size(2 * tw, 2 * th)  # ... superseded by the geometry
            e.set_input_geometry(g)
        streams.append([e.encode(*p) for p in pics])
        with pytest.raises(E.EncoderError):  # both setters: before the first submit only
            e.set_input_geometry(g)
        e.close()
    assert streams[0] == streams[1]
    # a later set_input_size supersedes the geometry: the stream of a handle that never had one
    big = nv12_clip(2 * tw, 2 * th, 2, 601)
    a = E.Encoder(tw, th, fixed_qp=QP, gop=GOP, geometry=E.geometry((iw, ih), dst=(28, 0, 38, 64)))
    a.set_input_size(2 * tw, 2 * th)
    with pytest.raises(E.EncoderError):
        a.set_crop(0, 0, 40, 40)  # (no geometry any more)
    b = E.Encoder(tw, th, fixed_qp=QP, gop=GOP, input_size=(2 * tw, 2 * th))
    assert [a.encode(*p) for p in big] == [b.encode(*p) for p in big]
    a.close(); b.close()


def _device_container(E, planes, rows, cols, stride, offset, seed):
    """the planes inside one device buffer that is noise everywhere else (between the rows too); -> (hip, buffer, plane pointers)"""
    from tests.inputref import hip as _hip
    hip = _hip()
    size = offset + sum(r * stride for r in rows) + 64
    host = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
    ptrs, o = [], offset
    for a, r, c in zip(planes, rows, cols):
        np.lib.stride_tricks.as_strided(host[o:], (r, c), (stride, 1))[:] = a
        ptrs.append(o)
        o += r * stride
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(size)) == 0
    assert hip.hipMemcpy(buf, host.ctypes.data_as(C.c_void_p), C.c_size_t(size), 1) == 0
    return hip, buf, [buf.value + p for p in ptrs]


def test_submit_device_reads_only_the_crop_at_an_odd_address_and_stride(E):
    """the caller's planes where they lie: an odd address, a stride that is no multiple of 4, noise between the rows and around the crop rectangle"""
    insize, crop, dst, (tw, th) = CASES["down-off-grid"]
    iw, ih = insize
    pics = nv12_clip(iw, ih, N, 700)
    ref = plain_stream(E, tw, th, geom_pictures(pics, insize, crop, dst, tw, th))
    rng = np.random.default_rng(701)
    for k in range(2):
        shown = [[np.ascontiguousarray(q) for q in _outside_replaced(G.FMT_NV12, list(p), iw, ih, crop, rng)] for p in pics]
        dev = [_device_container(E, p, [ih, ih // 2], [iw, iw], iw + 5, 3, 710 + 10 * k + i) for i, p in enumerate(shown)]
        e = encoder(E, CASES["down-off-grid"], keep_sar=True, pipeline_depth=2)  # (no aspect ratio in the SPS: the headers of the plain stream)
        got = run(e, lambda i: e.submit_device(dev[i][2][0], iw + 5, dev[i][2][1], iw + 5, pts=i), N)
        e.close()
        for hip, buf, _ in dev:
            hip.hipFree(buf)
        same(got, ref)


PAN = [(2 * i, 2 * i, 160 - 20 * i, 96 - 12 * i) for i in range(8)]  # a pan and a zoom at 5 : 3


def test_set_crop_in_flight(E):
    """three pictures in flight (the deepest pipeline), the crop changing before every submit: picture n is coded from geomref's picture of crop n"""
    iw, ih, tw, th = 160, 96, 80, 48
    pics = nv12_clip(iw, ih, len(PAN), 800)
    ref = plain_stream(E, tw, th, geom_pictures(pics, (iw, ih), PAN, (0, 0, tw, th), tw, th))
    e = E.Encoder(tw, th, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((iw, ih), crop=PAN[0], target=(tw, th)))
    got = run(e, lambda i: e.submit(*pics[i], pts=i), len(PAN), before=lambda i: e.set_crop(*PAN[i]))
    assert tuple(getattr(e.get_input_geometry(), k) for k in ("crop_x", "crop_y", "crop_w", "crop_h")) == PAN[-1]
    for bad in [(1, 0, 160, 96), (0, 0, 162, 96), (100, 0, 100, 60), (0, 0, 8, 6), (0, 0, 160, 48)]:  # odd, outside, outside, beyond 8, another aspect ratio
        with pytest.raises(E.EncoderError):
            e.set_crop(*bad)
    assert tuple(getattr(e.get_input_geometry(), k) for k in ("crop_x", "crop_y", "crop_w", "crop_h")) == PAN[-1]  # a refused crop changes nothing
    e.close()
    same(got, ref)
    assert spsref.sps_of(got[0][0][0])[0]["sar"] is None


def test_set_crop_in_flight_over_jpeg(E):
    data = open(JPEG, "rb").read()
    d = E.Encoder(72, 40, fixed_qp=QP)
    jy, juv = d.stage_jpeg(data)
    d.close()
    pic = (np.ascontiguousarray(jy[:40, :72]), np.ascontiguousarray(juv[:20, :72]))
    crops = [(0, 0, 72, 40), (2, 2, 54, 30), (4, 0, 36, 20), (0, 2, 18, 10), (18, 10, 54, 30), (36, 20, 36, 20), (54, 30, 18, 10), (0, 0, 72, 40)]  # 9 : 5
    ref = plain_stream(E, 72, 40, geom_pictures([pic] * 8, (72, 40), crops, (0, 0, 72, 40), 72, 40))
    e = E.Encoder(72, 40, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((72, 40), crop=crops[0], target=(72, 40)))
    got = run(e, lambda i: e.submit_jpeg(data, pts=i), 8, before=lambda i: e.set_crop(*crops[i]))
    e.close()
    same(got, ref)


def test_keep_sar_lets_the_crop_change_its_shape(E):
    iw, ih, tw, th = 160, 96, 80, 48
    pics = nv12_clip(iw, ih, 3, 900)
    crops = [(0, 0, 160, 96), (20, 0, 80, 96), (0, 30, 160, 40)]
    ref = plain_stream(E, tw, th, geom_pictures(pics, (iw, ih), crops, (0, 0, tw, th), tw, th))
    e = E.Encoder(tw, th, gop=GOP, fixed_qp=QP, pipeline_depth=2, geometry=E.geometry((iw, ih), target=(tw, th), keep_sar=True))
    got = run(e, lambda i: e.submit(*pics[i], pts=i), 3, before=lambda i: e.set_crop(*crops[i]))
    e.close()
    same(got, ref)
