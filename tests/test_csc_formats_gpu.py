"""GPU: the input formats of k_csc.hip (Y42B, Y444, YV12, NV21, RGB in six byte orders) bit-exact against tests/cscref.py -- the conversion
stage alone, on aligned and on unaligned planes, whole streams, and behind mi355enc_set_input_size -- and the colorimetry every SPS carries
(DESIGN.md section 11)."""
import os

import numpy as np
import pytest

from ceracoder_amd import synth
from oracle import csc as OC
from tests import cscref as R
from tests import scaleref as SR
from tests.spsref import nal_units, sps_of

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (64, 48), (322, 182), (1280, 720), (1920, 1080), (3840, 2160), (18, 34)]  # those of tests/test_csc_gpu.py
YUV_FMTS = [R.FMT_Y42B, R.FMT_Y444, R.FMT_YV12, R.FMT_NV21]
ids = lambda fmts: [R.NAMES[f] for f in fmts]


def same(got, want):
    assert np.array_equal(got[0], want[0]), ("luma", np.argwhere(got[0] != want[0])[:4])
    assert np.array_equal(got[1], want[1]), ("chroma", np.argwhere(got[1] != want[1])[:4])


# ---- the conversion stage
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", YUV_FMTS, ids=ids(YUV_FMTS))
def test_stage_csc_yuv_formats_match_numpy(E, fmt, w, h):
    e = E.Encoder(w, h, fixed_qp=30)
    planes = [np.ascontiguousarray(p) for p in R.random_planes(fmt, w, h, np.random.default_rng(fmt * 100 + w))]
    same(e.stage_csc(fmt, planes), R.to_nv12(fmt, planes, w, h))
    e.close()


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("fmt", R.RGB_FMTS, ids=ids(R.RGB_FMTS))
def test_stage_csc_rgb_formats_match_numpy_for_every_matrix_and_range(E, fmt, w, h):
    e = E.Encoder(w, h, fixed_qp=30)
    planes = [np.ascontiguousarray(p) for p in R.random_planes(fmt, w, h, np.random.default_rng(fmt * 100 + w))]
    sums = R.rgb_sums(fmt, planes[0], w, h)
    same(e.stage_csc(fmt, planes), R.to_nv12(fmt, planes, w, h))  # set_colorimetry never called: matrix by the coded size, limited range
    for m, fr in R.MATRIX_RANGE_PAIRS:
        e.set_colorimetry(fr, 2, 2, m)
        same(e.stage_csc(fmt, planes), R.pad_nv12(*R.rgb_convert(sums, R.coefficients(m, fr))))
    e.set_colorimetry(1, 1, 1, 2)  # unspecified matrix, full range
    same(e.stage_csc(fmt, planes), R.to_nv12(fmt, planes, w, h, matrix=2, full_range=1))
    e.close()


def _device(torch, planes, offset):
    """every plane in a device buffer of its own, `offset` bytes in and at the stride the host view has -> (tensors, addresses, strides)"""
    keep, ptrs, strides = [], [], []
    for p in planes:
        span = np.lib.stride_tricks.as_strided(p, ((p.shape[0] - 1) * p.strides[0] + p.shape[1],), (1,))  # the bytes from the first sample to the last
        t = torch.zeros(offset + span.size, dtype=torch.uint8, device="cuda")
        t[offset:] = torch.from_numpy(np.array(span))
        keep.append(t)
        ptrs.append(t.data_ptr() + offset)
        strides.append(p.strides[0])
    return keep, ptrs, strides


@pytest.mark.parametrize("pad,offset", [(5, 1), (3, 2), (1, 3), (0, 0)])
@pytest.mark.parametrize("fmt", R.NEW_FMTS, ids=ids(R.NEW_FMTS))
def test_unaligned_planes_on_the_device_take_the_bytewise_path(E, fmt, pad, offset):
    """Planes that start 1 - 3 bytes into their buffer with odd strides, converted where they lie (no repacking upload): the kernels' byte-wise
    path.  (0, 0): the same entry point on aligned planes."""
    import torch
    w, h = 322, 182
    e = E.Encoder(w, h, fixed_qp=30)
    if fmt in R.RGB_FMTS:
        e.set_colorimetry(1, 5, 6, 5)
    planes = R.random_planes(fmt, w, h, np.random.default_rng(fmt + 7 * pad), pad=pad, offset=offset)
    keep, ptrs, strides = _device(torch, planes, offset)
    W, H = e.mbw * 16, e.mbh * 16
    oy, ouv = torch.zeros(H * W, dtype=torch.uint8, device="cuda"), torch.zeros(H // 2 * W, dtype=torch.uint8, device="cuda")
    e.stage_csc_device(fmt, ptrs, strides, oy.data_ptr(), ouv.data_ptr())
    want = R.to_nv12(fmt, planes, w, h, matrix=5, full_range=1)
    same((oy.cpu().numpy().reshape(H, W), ouv.cpu().numpy().reshape(H // 2, W)), want)
    e.close()


def test_stage_csc_device_also_runs_the_existing_kernels(E):
    import torch
    w, h = 322, 182
    e = E.Encoder(w, h, fixed_qp=30)
    W, H = e.mbw * 16, e.mbh * 16
    for fmt in (OC.FMT_I420, OC.FMT_YUY2, OC.FMT_UYVY):
        planes = R.random_planes(fmt, w, h, np.random.default_rng(fmt), pad=3, offset=1)
        keep, ptrs, strides = _device(torch, planes, 1)
        oy, ouv = torch.zeros(H * W, dtype=torch.uint8, device="cuda"), torch.zeros(H // 2 * W, dtype=torch.uint8, device="cuda")
        e.stage_csc_device(fmt, ptrs, strides, oy.data_ptr(), ouv.data_ptr())
        same((oy.cpu().numpy().reshape(H, W), ouv.cpu().numpy().reshape(H // 2, W)), OC.to_nv12(fmt, planes, w, h))
    with pytest.raises(E.EncoderError, match=r"\(-1\)"):
        e.stage_csc_device(E.FMT_NV12, [oy.data_ptr(), ouv.data_ptr()], [W, W], oy.data_ptr(), ouv.data_ptr())
    e.close()


def test_y42b_on_the_device_equals_the_existing_yuy2_kernel(E):
    w, h = 1918, 1078
    e = E.Encoder(w, h, fixed_qp=30)
    y, u, v = (np.ascontiguousarray(p) for p in R.random_planes(R.FMT_Y42B, w, h, np.random.default_rng(5)))
    packed = np.empty((h, 2 * w), np.uint8)
    packed[:, 0::2], packed[:, 1::4], packed[:, 3::4] = y, u, v
    same(e.stage_csc(E.FMT_Y42B, [y, u, v]), e.stage_csc(E.FMT_YUY2, [packed]))
    e.close()


# ---- with an input size of its own
@pytest.mark.parametrize("geom", [((1920, 1080), (1280, 720)), ((1918, 1078), (642, 362)), ((640, 480), (80, 60))], ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
@pytest.mark.parametrize("fmt", R.NEW_FMTS, ids=ids(R.NEW_FMTS))
def test_scaled_input_is_conversion_then_the_nv12_scale(E, fmt, geom):
    (iw, ih), (ow, oh) = geom
    e = E.Encoder(ow, oh, fixed_qp=30, input_size=(iw, ih))
    planes = R.random_planes(fmt, iw, ih, np.random.default_rng(fmt + iw), pad=3, offset=1)
    cy, cuv = R.to_nv12(fmt, planes, iw, ih, coded=(ow, oh))
    want = SR.to_nv12(SR.FMT_NV12, [cy[:ih, :iw], cuv[:ih // 2, :iw]], iw, ih, ow, oh)
    same(e.stage_scale(fmt, planes), want)
    same(e.stage_csc(fmt, [np.ascontiguousarray(p) for p in planes]), want)
    e.close()


# ---- whole streams
def rgb_clip(w, h, n, bpp, order):
    """n packed RGB pictures with moving content, (h, bpp * w) each; order: the byte of R, G, B"""
    out = []
    for i, (y, uv) in enumerate(synth.s2_frames(w, h, n)):
        yy = y[:h, :w].astype(np.int32)
        u, v = (np.repeat(np.repeat(uv[:h // 2, k:w:2], 2, 0), 2, 1).astype(np.int32) - 128 for k in (0, 1))
        p = np.full((h, w, bpp), 255, np.uint8)
        p[:, :, order[0]] = np.clip(yy + (359 * v >> 8), 0, 255)
        p[:, :, order[1]] = np.clip(yy - (88 * u + 183 * v >> 8), 0, 255)
        p[:, :, order[2]] = np.clip(yy + (454 * u >> 8), 0, 255)
        out.append(p.reshape(h, bpp * w))
    return out


def drain(e, depth, feed, n):
    aus = []
    for i in range(n):
        feed(i)
        if e.pending > depth:
            aus.append(e.collect()[:2])
    while e.pending:
        aus.append(e.collect()[:2])
    return aus


@pytest.mark.parametrize("depth,pinned", [(0, False), (2, False), (2, True)], ids=["depth0", "depth2", "depth2-pinned"])
@pytest.mark.parametrize("fmt", [R.FMT_BGRX, R.FMT_RGB], ids=["BGRx", "RGB"])
def test_rgb_stream_equals_the_stream_of_its_converted_pictures(E, oracle, fmt, depth, pinned):
    w, h, n = 322, 182, 10
    bpp, ro, go, bo = R.RGB_LAYOUT[fmt]
    clip = rgb_clip(w, h, n, bpp, (ro, go, bo))
    a, b = E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=depth), E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=depth)
    conv = [R.to_nv12(fmt, [p], w, h) for p in clip]
    bufs = [E.PinnedBuffer(h * bpp * w) for _ in range(depth + 1)] if pinned else None

    def feed_rgb(i):
        p = clip[i]
        if pinned:
            view = bufs[i % len(bufs)].array.reshape(h, bpp * w)
            view[:] = p
            p = view
        a.submit_fmt(fmt, [p], pts=i)
    got = drain(a, depth, feed_rgb, n)
    ref = drain(b, depth, lambda i: b.submit(conv[i][0][:h, :w], conv[i][1][:h // 2, :w], pts=i), n)
    assert got == ref and [k for _, k in got] == [i % 4 == 0 for i in range(n)]
    dec = oracle.Decoder()
    for au, _ in got:
        y, uv = dec.decode(au)
    assert np.array_equal(y, a.fetch(E.FETCH_RECON_Y)) and np.array_equal(uv, a.fetch(E.FETCH_RECON_UV))
    a.close(); b.close()
    for p in bufs or []:
        p.free()


def test_y42b_stream_equals_yuy2_stream(E):
    w, h, n = 322, 182, 6
    a, b = E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=1), E.Encoder(w, h, gop=4, fixed_qp=28, pipeline_depth=1)
    rng = np.random.default_rng(2)
    pics = []
    for y, uv in synth.s2_frames(w, h, n):
        u = np.repeat(uv[:h // 2, 0:w:2], 2, 0) + rng.integers(0, 3, (h, w // 2), dtype=np.uint8)  # (full-height chroma whose two rows differ)
        v = np.repeat(uv[:h // 2, 1:w:2], 2, 0) + rng.integers(0, 3, (h, w // 2), dtype=np.uint8)
        pics.append((np.ascontiguousarray(y[:h, :w]), u, v))

    def packed(i):
        y, u, v = pics[i]
        p = np.empty((h, 2 * w), np.uint8)
        p[:, 0::2], p[:, 1::4], p[:, 3::4] = y, u, v
        return p
    got = drain(a, 1, lambda i: a.submit_fmt(E.FMT_Y42B, list(pics[i]), pts=i), n)
    ref = drain(b, 1, lambda i: b.submit_fmt(E.FMT_YUY2, [packed(i)], pts=i), n)
    assert got == ref
    a.close(); b.close()


# ---- colorimetry
def sps_list(aus):
    return [s for au in aus for s in sps_of(au)]


@pytest.mark.parametrize("col", [(0, 1, 1, 1), (1, 2, 2, 6), (1, 2, 2, 2), (0, 9, 16, 9)])
def test_every_sps_carries_the_colorimetry(E, oracle, col):
    w, h, n = 320, 192, 9
    clip = list(synth.s2_frames(w, h, n))
    for kw in ({}, {"intra_refresh": True}, {"transform8x8": True}):
        e = E.Encoder(w, h, gop=4, fixed_qp=30, colorimetry=col, **kw)
        dec, aus = oracle.Decoder(), []
        for i, (y, uv) in enumerate(clip):
            au, key = e.encode(y, uv, pts=i)
            aus.append(au)
            dy, duv = dec.decode(au)
            assert (7 in [t for t, _, _ in nal_units(au)]) == key
        assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
        got = sps_list(aus)
        assert len(got) == sum(7 in [t for t, _, _ in nal_units(au)] for au in aus) >= 2 and all(s["colorimetry"] == col for s in got), kw
        with pytest.raises(E.EncoderError, match=r"\(-6\)"):
            e.set_colorimetry(0, 1, 1, 1)
        e.close()


def test_recovery_reencode_carries_the_colorimetry(E):
    w, h, n = 640, 368, 10
    clip = list(synth.s2_frames(w, h, n))
    e = E.Encoder(w, h, gop=40, fixed_qp=30, pipeline_depth=2, exclusive=True, colorimetry=(1, 1, 13, 5))
    out = []
    for i, (y, uv) in enumerate(clip):
        if i == 5:
            e.debug_trip_wait(12)
        e.submit(y, uv, pts=i)
        if e.pending > 2:
            out.append(e.collect())
    while e.pending:
        out.append(e.collect())
    assert e.stats().recoveries == 1 and [i for i, o in enumerate(out) if o[1]] == [0, 5]
    got = sps_list([o[0] for o in out])
    assert len(got) == 2 and all(s["colorimetry"] == (1, 1, 13, 5) for s in got)
    e.close()


def test_setter_arguments_and_matrices_rgb_cannot_use(E):
    w, h = 64, 48
    e = E.Encoder(w, h, fixed_qp=30)
    for bad in ((2, 1, 1, 1), (-1, 1, 1, 1), (0, 256, 1, 1), (0, 1, -1, 1), (0, 1, 1, 256)):
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.set_colorimetry(*bad)
    rgb = np.zeros((h, 4 * w), np.uint8)
    y, uv = np.zeros((h, w), np.uint8), np.full((h // 2, w), 128, np.uint8)
    for m in (0, 8):
        e.set_colorimetry(0, 1, 1, m)
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.submit_fmt(E.FMT_BGRX, [rgb])
        with pytest.raises(E.EncoderError, match=r"\(-1\)"):
            e.stage_csc(E.FMT_RGBX, [rgb])
        assert e.pending == 0
    au, key = e.encode(y, uv)  # YUV input is only labelled: any code point goes
    assert key and sps_of(au)[0]["colorimetry"] == (0, 1, 1, 8)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.set_colorimetry(0, 1, 1, 1)
    e.close()


@pytest.mark.parametrize("fmt", [OC.FMT_NV12, OC.FMT_I420, OC.FMT_YUY2, OC.FMT_UYVY], ids=["nv12", "i420", "yuy2", "uyvy"])
def test_without_the_setter_the_old_formats_give_the_old_stream(E, fmt):
    """No video_signal_type, the parameter sets of mi355enc_host_write_headers, and the access units of an encoder fed the NV12 pictures
    oracle/csc.py (frozen) makes of the same input -- with (0, 2, 2, 2) set explicitly as well."""
    w, h, n = 322, 182, 6
    rng = np.random.default_rng(fmt)
    hdr = E.host_write_headers(w, h, 60)
    streams = []
    for col in (None, (0, 2, 2, 2)):
        a, b = E.Encoder(w, h, gop=4, fixed_qp=28, colorimetry=col), E.Encoder(w, h, gop=4, fixed_qp=28)
        for i, (y, uv) in enumerate(synth.s2_frames(w, h, n)):
            yy, cc = np.ascontiguousarray(y[:h, :w]), np.ascontiguousarray(uv[:h // 2, :w])
            if fmt == OC.FMT_NV12:
                planes, conv = [yy, cc], (yy, cc)
            else:
                if fmt == OC.FMT_I420:
                    planes = [yy, np.ascontiguousarray(cc[:, 0::2]), np.ascontiguousarray(cc[:, 1::2])]
                else:
                    p = np.empty((h, 2 * w), np.uint8)
                    yo, uo, vo = (0, 1, 3) if fmt == OC.FMT_YUY2 else (1, 0, 2)
                    p[:, yo::2] = yy
                    p[:, uo::4], p[:, vo::4] = np.repeat(cc[:, 0::2], 2, 0), np.repeat(cc[:, 1::2], 2, 0)
                    planes = [p]
                oy, ouv = OC.to_nv12(fmt, planes, w, h)
                conv = (oy[:h, :w], ouv[:h // 2, :w])
            a.submit_fmt(fmt, planes, pts=i)
            au, key = a.collect()[:2]
            ref, _ = b.encode(conv[0], conv[1], pts=i)
            assert au == ref, i
            assert au.startswith(hdr) == key
            streams.append(au)
        a.close(); b.close()
    assert streams[:n] == streams[n:]


# ---- the element
def _harness():
    from tests.test_boundary_cpu import HARNESS
    return HARNESS


def _element(tmp_path, name, caps, n=4):
    """videotestsrc ! caps ! mi355h264enc ! appsink through the reference's pipeline loader -> the access units"""
    import subprocess
    from tests.test_boundary_cpu import HARNESS, gst_env
    from tests.test_gst_gpu import read_records
    pf = tmp_path / ("pipe_" + name)
    pf.write_text("videotestsrc num-buffers=%d ! video/x-raw,framerate=30/1,%s ! mi355h264enc key-int-max=30 qp=24 name=venc_bps ! "
                  "appsink name=appsink sync=false\n" % (n, caps))
    out = tmp_path / ("out_%s.bin" % name)
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return [au for _, au in read_records(str(out))]


@pytest.mark.skipif(not os.path.exists(_harness()), reason="oracle/_ref/ref_harness not shipped")
@pytest.mark.parametrize("fmt", ["Y42B", "Y444", "BGRx", "RGB", "YV12", "NV21", "ARGB"])
def test_element_takes_the_new_formats_without_videoconvert(tmp_path, oracle, fmt):
    aus = _element(tmp_path, fmt, "width=320,height=180,format=%s" % fmt)
    assert len(aus) == 4
    dec = oracle.Decoder()
    for au in aus:
        y, uv = dec.decode(au)
    assert dec.size == (320, 180)
    # SMPTE bars: white-ish at the left, blue at the right of the upper part; chroma of the grey bar is neutral
    assert float(y[20:100, 4:40].mean()) > 150 and float(y[20:100, 280:310].mean()) < 70
    assert abs(float(uv[10:50, 4:40].mean()) - 128) < 6
    cb, cr = uv[10:50, 280:310:2], uv[10:50, 281:310:2]
    assert float(cb.mean()) > 180 and float(cr.mean()) < 128  # blue
    (s,) = sps_of(aus[0])
    assert s["colorimetry"] == (0, 6, 6, 6)  # below 1024 x 576: BT.601, limited range -- chosen for RGB, videotestsrc's default for YUV


@pytest.mark.skipif(not os.path.exists(_harness()), reason="oracle/_ref/ref_harness not shipped")
@pytest.mark.parametrize("caps,want", [("width=320,height=192,format=I420,colorimetry=(string)bt601", (0, 6, 6, 6)),
                                       ("width=320,height=192,format=I420,colorimetry=(string)bt709", (0, 1, 1, 1)),
                                       ("width=320,height=192,format=Y42B,colorimetry=(string)1:4:0:0", (1, 2, 2, 6)),
                                       ("width=1280,height=720,format=BGRx", (0, 1, 1, 1)),
                                       ("width=640,height=480,format=RGB", (0, 6, 6, 6))],
                         ids=["bt601", "bt709", "jpeg", "bgrx-720p", "rgb-480p"])
def test_element_signals_the_caps_colorimetry(tmp_path, caps, want):
    aus = _element(tmp_path, "col", caps, n=2)
    (s,) = sps_of(aus[0])
    assert s["colorimetry"] == want
