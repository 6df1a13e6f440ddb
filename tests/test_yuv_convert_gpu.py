"""GPU: the colour step (YUV of one range and matrix -> another, in place on the coded surfaces) and the 10-bit / grey input formats, bit-exact against
tests/yuvref.py: the stages alone, under a geometry and an orientation, on unaligned planes, behind mi355enc_set_input_size, and whole streams through every
submit entry point."""
import ctypes as C
import os

import numpy as np
import pytest

from ceracoder_amd import synth
from oracle import csc as OC
from tests import cscref as CR
from tests import scaleref as SR
from tests import yuvref as R
from tests.spsref import sps_of
from tests.inputref import device_free, hip
from tests.test_csc_formats_gpu import drain, rgb_clip, same

pytestmark = pytest.mark.gpu

JPEG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpeg", "q50_420_72x40.jpg")
SIZES = [(16, 16), (18, 34), (64, 48), (322, 182)]
# (input (full, matrix), output colorimetry (full, primaries, transfer, matrix))
PAIRS = {"full601-lim709": ((1, 6), (0, 1, 1, 1)), "lim601-lim709": ((0, 6), (0, 1, 1, 1)), "lim709-full709": ((0, 1), (1, 1, 1, 1)), "full2020-lim601": ((1, 9), (0, 6, 6, 6))}
IN, COL = PAIRS["full601-lim709"]  # what the stream tests run with: JPEG's samples to what an ingest assumes
COEF = R.coefficients(IN[1], IN[0], COL[3], COL[0])
DEEP_IDS = [R.NAMES[f] for f in R.DEEP_FMTS]


def coef_of(pair):
    (ifr, im), (ofr, _, _, om) = pair
    return R.coefficients(im, ifr, om, ofr)


def dev_put(a, offset=0):
    """the bytes of `a` in device memory of their own, `offset` bytes into the buffer -> the buffer's address (hipMalloc: 256-byte aligned)"""
    a = np.ascontiguousarray(a)
    d = C.c_void_p()
    assert hip().hipMalloc(C.byref(d), C.c_size_t(offset + a.nbytes)) == 0
    assert hip().hipMemcpy(C.c_void_p(d.value + offset), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0  # hipMemcpyHostToDevice, synchronous
    return d.value


def dev_get(ptr, shape):
    out = np.empty(shape, np.uint8)
    assert hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return out


def noise(w, h, seed):
    """coded-size planes of full-byte-range noise: every clip happens"""
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    rng = np.random.default_rng(seed)
    y, uv = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H // 2, W), dtype=np.uint8)
    for k in range(8):  # ... and the eight corners of the cube, one 2 x 2 block each, whatever the seed
        y[0:2, 2 * k:2 * k + 2], uv[0, 2 * k], uv[0, 2 * k + 1] = 255 * (k & 1), 255 * (k >> 1 & 1), 255 * (k >> 2)
    return y, uv


# ---- the colour step alone
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("pair", list(PAIRS), ids=list(PAIRS))
def test_stage_yuv_convert_matches_numpy(E, pair, w, h):
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=PAIRS[pair][1], input_colorimetry=PAIRS[pair][0])
    y, uv = noise(w, h, w + len(pair))
    want = R.convert(y, uv, coef_of(PAIRS[pair]))
    raw = R.unclipped(coef_of(PAIRS[pair]), y[0:2, 0:16], np.repeat(np.repeat(uv[0:1, 0:16:2], 2, 0), 2, 1), np.repeat(np.repeat(uv[0:1, 1:16:2], 2, 0), 2, 1))[0]
    assert raw.min() < 0 and raw.max() > 255  # (both clips are exercised)
    same(e.stage_yuv_convert(y, uv), want)
    e.close()


def test_stage_yuv_convert_1080p(E):
    w, h = 1920, 1080
    e = E.Encoder(w, h, fixed_qp=30, input_colorimetry=(1, 6))  # the output never set: unspecified, BT.709 by the size, limited range
    y, uv = noise(w, h, 3)
    same(e.stage_yuv_convert(y, uv), R.convert(y, uv, R.coefficients(6, 1, 1, 0)))
    e.set_input_colorimetry(0, 2)  # both unspecified: equal
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stage_yuv_convert(y, uv)
    e.close()


@pytest.mark.parametrize("method", [0, 1, 2, 6], ids=["none", "90r", "180", "ul-lr"])
def test_under_a_geometry_the_border_keeps_its_bytes(E, method):
    """A letterbox inside the picture (the margin is border), one that reaches the target's right and bottom edge, and one that reaches its left and top edge
    (under a flip: the coded picture's right and bottom, so the margin is picture)."""
    w, h = 322, 182
    tw, th = (h, w) if method in R.TRANSPOSING else (w, h)
    margin_is_picture = []
    for k, dst in enumerate([(42, 10, tw - 90, th - 40), (10, 12, tw - 10, th - 12), (0, 0, tw - 10, th - 12)]):
        e = E.Encoder(w, h, fixed_qp=30, colorimetry=COL, input_colorimetry=IN, orientation=method or None, geometry=E.geometry((160, 96), dst=dst))
        y, uv = noise(w, h, 10 * method + k)
        mask = R.picture_mask(w, h, dst, method)
        assert mask.any() and not mask.all()
        margin_is_picture.append(bool(mask[h:, :].any() or mask[:, w:].any()))
        got = e.stage_yuv_convert(y, uv)
        same(got, R.convert(y, uv, COEF, mask))
        assert np.array_equal(got[0][~mask], y[~mask]) and not np.array_equal(got[0][mask], y[mask])
        e.close()
    assert not margin_is_picture[0] and any(margin_is_picture[1:])


# ---- the formats
@pytest.mark.parametrize("w,h", SIZES + [(1920, 1080)])
@pytest.mark.parametrize("fmt", R.DEEP_FMTS, ids=DEEP_IDS)
def test_stage_csc_deep_formats_match_numpy(E, fmt, w, h):
    e = E.Encoder(w, h, fixed_qp=30)
    planes = [np.ascontiguousarray(p) for p in R.random_planes(fmt, w, h, np.random.default_rng(fmt * 100 + w))]
    same(e.stage_csc(fmt, planes), R.to_nv12(fmt, planes, w, h))
    e.close()


def test_the_mirror_takes_wide_planes_as_words(E):
    w, h = 64, 48
    e = E.Encoder(w, h, fixed_qp=30)
    planes = [np.ascontiguousarray(p) for p in R.random_planes(R.FMT_P010, w, h, np.random.default_rng(1))]
    same(e.stage_csc(E.FMT_P010, [p.view("<u2") for p in planes]), R.to_nv12(R.FMT_P010, planes, w, h))
    e.close()


@pytest.mark.parametrize("pad,offset", [(5, 1), (3, 2), (1, 3), (0, 0)])
@pytest.mark.parametrize("fmt", R.DEEP_FMTS, ids=DEEP_IDS)
def test_unaligned_deep_planes_on_the_device(E, fmt, pad, offset):
    w, h = 322, 182
    e = E.Encoder(w, h, fixed_qp=30)
    planes = R.random_planes(fmt, w, h, np.random.default_rng(fmt + 7 * pad), pad=pad, offset=offset)
    # every plane in a device buffer of its own, `offset` bytes in and at the stride the host view has: the bytes from its first sample to its last
    bufs = [dev_put(np.lib.stride_tricks.as_strided(p, ((p.shape[0] - 1) * p.strides[0] + p.shape[1],), (1,)), offset) for p in planes]
    W, H = e.mbw * 16, e.mbh * 16
    oy, ouv = dev_put(np.zeros(H * W, np.uint8)), dev_put(np.zeros(H // 2 * W, np.uint8))
    e.stage_csc_device(fmt, [b + offset for b in bufs], [p.strides[0] for p in planes], oy, ouv)
    same((dev_get(oy, (H, W)), dev_get(ouv, (H // 2, W))), R.to_nv12(fmt, planes, w, h))
    e.close()
    for d in bufs + [oy, ouv]:
        device_free(d)


@pytest.mark.parametrize("geom", [((1918, 1078), (642, 362)), ((640, 480), (80, 60))], ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
@pytest.mark.parametrize("fmt", R.DEEP_FMTS, ids=DEEP_IDS)
def test_scaled_deep_input_is_conversion_then_the_nv12_scale(E, fmt, geom):
    (iw, ih), (ow, oh) = geom
    e = E.Encoder(ow, oh, fixed_qp=30, input_size=(iw, ih))
    planes = R.random_planes(fmt, iw, ih, np.random.default_rng(fmt + iw), pad=3, offset=1)
    cy, cuv = R.to_nv12(fmt, planes, iw, ih)
    want = SR.to_nv12(SR.FMT_NV12, [cy[:ih, :iw], cuv[:ih // 2, :iw]], iw, ih, ow, oh)
    same(e.stage_scale(fmt, planes), want)
    same(e.stage_csc(fmt, [np.ascontiguousarray(p) for p in planes]), want)
    e.close()


# ---- whole streams
N, GOP, QP = 6, 4, 28


def clip(w, h):
    return [(np.ascontiguousarray(y[:h, :w]), np.ascontiguousarray(uv[:h // 2, :w])) for y, uv in synth.s2_frames(w, h, N)]


def in_fmt(E, fmt, y, uv, rng):
    """an NV12 picture in `fmt` -> (planes to submit, the coded NV12 surfaces the format's own conversion makes of them)"""
    h, w = y.shape
    u, v = uv[:, 0::2], uv[:, 1::2]
    u2, v2 = (np.repeat(c, 2, 0) + rng.integers(0, 3, (h, w // 2), dtype=np.uint8) for c in (u, v))  # full-height chroma whose two rows differ
    if fmt == E.FMT_NV12:
        return [y, uv], CR.pad_nv12(y, u, v)
    if fmt == E.FMT_I420:
        planes = [y, np.ascontiguousarray(u), np.ascontiguousarray(v)]
        return planes, OC.to_nv12(fmt, planes, w, h)
    if fmt == E.FMT_YUY2:
        p = np.empty((h, 2 * w), np.uint8)
        p[:, 0::2], p[:, 1::4], p[:, 3::4] = y, u2, v2
        return [p], OC.to_nv12(fmt, [p], w, h)
    if fmt == E.FMT_Y42B:
        return [y, u2, v2], CR.to_nv12(fmt, [y, u2, v2], w, h)
    low = lambda c: (c.astype(np.int64) << 2) | rng.integers(0, 4, c.shape)  # ten bits that round to other bytes than the eight they came from
    if fmt == E.FMT_P010:
        c10 = np.empty((h // 2, w), np.int64)
        c10[:, 0::2], c10[:, 1::2] = low(u), low(v)
        planes = [np.ascontiguousarray((p << 6).astype("<u2")).view(np.uint8) for p in (low(y), c10)]
    elif fmt == E.FMT_V210:
        planes = [R.pack_v210(low(y), low(u2), low(v2), rng)]
    else:
        raise ValueError(fmt)
    return planes, R.to_nv12(fmt, planes, w, h)


def feed_converted(b, conv, w, h):
    return lambda i: b.submit(conv[i][0][:h, :w], conv[i][1][:h // 2, :w], pts=i)


def pair_of_encoders(E, w, h, depth, **kw):
    """a: converts on the way in; b: is fed the converted pictures; the same output colorimetry"""
    return (E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, colorimetry=COL, input_colorimetry=IN, **kw),
            E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, colorimetry=COL, **kw))


def check_streams(got, ref):
    assert [k for _, k in got] == [i % GOP == 0 for i in range(N)]
    assert got == ref


STREAM_FMTS = ["NV12", "I420", "YUY2", "Y42B", "P010", "V210"]


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("w,h", [(64, 48), (322, 182)])
@pytest.mark.parametrize("name", STREAM_FMTS)
def test_converting_stream_equals_the_stream_of_the_converted_pictures(E, name, w, h, depth):
    fmt = getattr(E, "FMT_" + name)
    rng = np.random.default_rng(w + fmt)
    made = [in_fmt(E, fmt, y, uv, rng) for y, uv in clip(w, h)]
    conv = [R.convert(cy, cuv, COEF) for _, (cy, cuv) in made]
    a, b = pair_of_encoders(E, w, h, depth)
    if fmt == E.FMT_NV12:
        got = drain(a, depth, lambda i: a.submit(*made[i][0], pts=i), N)
    else:
        got = drain(a, depth, lambda i: a.submit_fmt(fmt, made[i][0], pts=i), N)
    check_streams(got, drain(b, depth, feed_converted(b, conv, w, h), N))
    assert got != drain_plain(E, w, h, depth, made)  # (the step does something)
    (s,) = sps_of(got[0][0])
    assert s["colorimetry"] == COL  # the output's codes, not the input's
    a.close(); b.close()


def drain_plain(E, w, h, depth, made):
    c = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, colorimetry=COL)
    out = drain(c, depth, lambda i: c.submit(made[i][1][0][:h, :w], made[i][1][1][:h // 2, :w], pts=i), N)
    c.close()
    return out


@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("w,h", [(64, 48), (322, 182)])
def test_submit_device_converts_and_leaves_the_callers_planes_alone(E, w, h, depth):
    """64 x 48 on aligned planes would take the in-place exit: with a conversion it must not, and the planes stay what they were"""
    pics = clip(w, h)
    conv = [R.convert(*CR.pad_nv12(y, uv[:, 0::2], uv[:, 1::2]), COEF) for y, uv in pics]
    dev = [(dev_put(y), dev_put(uv)) for y, uv in pics]
    a, b = pair_of_encoders(E, w, h, depth)
    got = drain(a, depth, lambda i: a.submit_device(dev[i][0], w, dev[i][1], w, pts=i), N)
    check_streams(got, drain(b, depth, feed_converted(b, conv, w, h), N))
    for (dy, duv), (y, uv) in zip(dev, pics):
        assert np.array_equal(dev_get(dy, y.shape), y) and np.array_equal(dev_get(duv, uv.shape), uv)
    a.close(); b.close()
    for dy, duv in dev:
        device_free(dy); device_free(duv)


@pytest.mark.parametrize("depth", [0, 2])
def test_submit_jpeg_converts(E, depth):
    data = open(JPEG, "rb").read()
    w, h = 72, 40
    plain = E.Encoder(w, h, fixed_qp=QP)
    conv = [R.convert(*plain.stage_jpeg(data), COEF)] * N
    plain.close()
    a, b = pair_of_encoders(E, w, h, depth)
    got = drain(a, depth, lambda i: a.submit_jpeg(data, pts=i), N)
    check_streams(got, drain(b, depth, feed_converted(b, conv, w, h), N))
    a.close(); b.close()


def test_layers_and_text_are_drawn_behind_the_step_in_the_outputs_colours(E):
    w, h, depth = 322, 182, 2
    pics = clip(w, h)
    conv = [R.convert(*CR.pad_nv12(y, uv[:, 0::2], uv[:, 1::2]), COEF) for y, uv in pics]
    rng = np.random.default_rng(5)
    logo = rng.integers(0, 256, (40, 60, 4), dtype=np.uint8)
    a, b = pair_of_encoders(E, w, h, depth)
    for e in (a, b):
        e.set_image(0, logo, x=30, y=20)
        e.set_overlay_text("colour 12:34")
    got = drain(a, depth, lambda i: a.submit(*pics[i], pts=i), N)
    check_streams(got, drain(b, depth, feed_converted(b, conv, w, h), N))
    a.close(); b.close()


def test_geometry_and_orientation_stream(E):
    """scale + letterbox + 90r, then the step on the picture part only: the stream of a plain handle fed the masked conversion of what the geometry makes"""
    w, h, depth, dst = 182, 322, 2, (42, 10, 232, 150)  # pre-orientation target 322 x 182
    geom = dict(orientation="90r", geometry=E.geometry((160, 96), dst=dst, keep_sar=True))
    pics = clip(160, 96)
    c = E.Encoder(w, h, fixed_qp=QP, **geom)
    mask = R.picture_mask(w, h, dst, 1)
    conv = [R.convert(*c.stage_geometry(E.FMT_NV12, list(p)), COEF, mask) for p in pics]
    c.close()
    a = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, colorimetry=COL, input_colorimetry=IN, **geom)
    b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, colorimetry=COL)
    got = drain(a, depth, lambda i: a.submit(*pics[i], pts=i), N)
    check_streams(got, drain(b, depth, feed_converted(b, conv, w, h), N))
    a.close(); b.close()


def test_a_recovery_does_not_convert_twice(E):
    w, h, n = 640, 368, 8
    pics = [(np.ascontiguousarray(y[:h, :w]), np.ascontiguousarray(uv[:h // 2, :w])) for y, uv in synth.s2_frames(w, h, n)]
    conv = [R.convert(y, uv, COEF) for y, uv in pics]
    kw = dict(gop=40, fixed_qp=30, pipeline_depth=2, exclusive=True, colorimetry=COL)
    a, b = E.Encoder(w, h, input_colorimetry=IN, **kw), E.Encoder(w, h, **kw)

    def run(e, src):
        out = []
        for i in range(n):
            if i == 4:
                e.debug_trip_wait(12)
            e.submit(*src[i], pts=i)
            if e.pending > 2:
                out.append(e.collect()[:2])
        while e.pending:
            out.append(e.collect()[:2])
        assert e.stats().recoveries == 1
        return out
    assert run(a, pics) == run(b, conv)
    a.close(); b.close()


# ---- what stays as it was
def test_an_input_equal_to_the_output_adds_nothing(E):
    w, h = 64, 48
    pics = clip(w, h)
    for col, inp in (((0, 1, 1, 1), (0, 1)), (None, (0, 6)), (None, (0, 2)), ((1, 2, 2, 5), (1, 6))):
        a, b = E.Encoder(w, h, gop=GOP, fixed_qp=QP, colorimetry=col, input_colorimetry=inp), E.Encoder(w, h, gop=GOP, fixed_qp=QP, colorimetry=col)
        with pytest.raises(E.EncoderError, match=r"\(-6\)"):
            a.stage_yuv_convert(*noise(w, h, 1))
        assert drain(a, 0, lambda i: a.submit(*pics[i], pts=i), N) == drain(b, 0, lambda i: b.submit(*pics[i], pts=i), N)
        a.close(); b.close()
    e = E.Encoder(w, h, fixed_qp=QP)  # the call never made: no step either
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stage_yuv_convert(*noise(w, h, 1))
    e.close()


def test_rgb_input_is_not_touched_by_the_input_colorimetry(E):
    w, h = 322, 182
    pics = rgb_clip(w, h, N, 4, (2, 1, 0))
    a, b = pair_of_encoders(E, w, h, 2)
    assert drain(a, 2, lambda i: a.submit_fmt(E.FMT_BGRX, [pics[i]], pts=i), N) == drain(b, 2, lambda i: b.submit_fmt(E.FMT_BGRX, [pics[i]], pts=i), N)
    a.close(); b.close()


def test_setter_arguments_state_and_outputs_the_step_cannot_reach(E):
    w, h = 64, 48
    y, uv = clip(w, h)[0]
    e = E.Encoder(w, h, fixed_qp=QP)
    for bad in ((2, 1), (-1, 1), (0, 0), (0, 3), (0, 4), (0, 7), (0, 8), (0, 10), (0, 256)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_input_colorimetry(*bad)
    e.set_input_colorimetry(1, 6)
    e.set_colorimetry(0, 1, 1, 4)  # (either order) an output matrix the step cannot convert to
    dy, duv = dev_put(y), dev_put(uv)
    for submit in (lambda: e.submit(y, uv), lambda: e.submit_fmt(E.FMT_I420, [y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])]),
                   lambda: e.submit_fmt(E.FMT_GRAY8, [y]), lambda: e.submit_device(dy, w, duv, w),
                   lambda: e.submit_jpeg(open(JPEG, "rb").read())):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            submit()
        assert e.pending == 0
    e.set_colorimetry(0, 1, 1, 1)
    au, key = e.encode(y, uv)
    assert key and sps_of(au)[0]["colorimetry"] == (0, 1, 1, 1)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.set_input_colorimetry(0, 1)
    e.close()
    device_free(dy); device_free(duv)
