"""GPU: downscaling on the way in (mi355enc_set_input_size, k_scale.hip) -- the kernel bit-exact against tests/scaleref.py, streams
submitted at the input size equal to the same pictures scaled by numpy and submitted unscaled, the SPS's sample aspect ratio, the call
order, and the element's width / height."""
import os
import subprocess

import numpy as np
import pytest

from tests import scaleref as R
from tests.inputref import device_planes

pytestmark = pytest.mark.gpu

FMTS = [R.FMT_NV12, R.FMT_I420, R.FMT_YUY2, R.FMT_UYVY]
GEOMS = [((3840, 2160), (1920, 1080)), ((3840, 2160), (1280, 720)), ((3840, 2160), (640, 360)), ((1920, 1080), (1280, 720)),
         ((1920, 1080), (854, 480)), ((2560, 1440), (1920, 1080)), ((1280, 720), (160, 90)),
         ((1918, 1078), (642, 362)), ((640, 480), (80, 60)), ((64, 48), (64, 48)), ((1920, 1080), (1920, 1072))]


def planes_of(fmt, w, h, rng, pad=0, offset=0):
    """random planes of a w x h picture in `fmt`; pad: extra bytes per row (the stride), offset: the first sample's offset in its buffer"""
    def mk(rows, cols):
        buf = rng.integers(0, 256, rows * (cols + pad) + offset, dtype=np.uint8)
        return np.lib.stride_tricks.as_strided(buf[offset:], (rows, cols), (cols + pad, 1))
    if fmt == R.FMT_NV12:
        return [mk(h, w), mk(h // 2, w)]
    if fmt == R.FMT_I420:
        return [mk(h, w), mk(h // 2, w // 2), mk(h // 2, w // 2)]
    return [mk(h, 2 * w)]


@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
@pytest.mark.parametrize("fmt", FMTS, ids=["nv12", "i420", "yuy2", "uyvy"])
def test_stage_scale_is_bit_exact(E, fmt, geom):
    (iw, ih), (ow, oh) = geom
    e = E.Encoder(ow, oh, fixed_qp=30, input_size=(iw, ih))
    pl = planes_of(fmt, iw, ih, np.random.default_rng(iw * 7 + ow + fmt))
    dy, duv = e.stage_scale(fmt, pl)
    ry, ruv = R.to_nv12(fmt, pl, iw, ih, ow, oh)
    assert np.array_equal(dy, ry), np.argwhere(dy != ry)[:4]
    assert np.array_equal(duv, ruv), np.argwhere(duv != ruv)[:4]
    e.close()


def test_device_tables_are_the_host_tables(E):
    e = E.Encoder(642, 362, fixed_qp=30, input_size=(1918, 1078))
    dev = e.scale_tables_device()
    spec = [(1918, 642, R.LUMA), (1078, 362, R.LUMA), (1918, 642, R.CHROMA_H), (1078, 362, R.CHROMA_V), (1078, 362, R.CHROMA_V422)]
    for (f, c), a in zip(dev, spec):
        hf, hc = E.scale_table(*a)
        assert np.array_equal(f, hf) and np.array_equal(c, hc), a
    e.close()


@pytest.mark.parametrize("fmt", FMTS, ids=["nv12", "i420", "yuy2", "uyvy"])
def test_strided_and_misaligned_planes(E, fmt):
    """Row strides that are not multiples of 4 and planes that start at an odd address: the host copy packs them; the result is the same."""
    iw, ih, ow, oh = 1922, 1082, 960, 540
    e = E.Encoder(ow, oh, fixed_qp=30, input_size=(iw, ih))
    pl = planes_of(fmt, iw, ih, np.random.default_rng(5 + fmt), pad=7, offset=1)
    dy, duv = e.stage_scale(fmt, pl)
    ry, ruv = R.to_nv12(fmt, pl, iw, ih, ow, oh)
    assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
    e.close()


def test_stage_scale_before_set_input_size_is_refused(E):
    e = E.Encoder(320, 192, fixed_qp=30)
    with pytest.raises(E.EncoderError, match=r"\(-6\)"):
        e.stage_scale(R.FMT_I420, planes_of(R.FMT_I420, 320, 192, np.random.default_rng(1)))
    e.close()


# ---- streams
def clip(w, h, n, seed=3):
    """n NV12 pictures of w x h: smooth shapes that move, some texture (content the coder has to work on)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    tex = rng.integers(0, 24, (h, w)).astype(np.float32)
    out = []
    for i in range(n):
        y = 110 + 60 * np.sin((xx + 9 * i) / (w / 7.0)) * np.cos((yy - 5 * i) / (h / 5.0)) + tex
        cx, cy = w * (0.3 + 0.05 * i), h * 0.5
        y = np.where((xx - cx) ** 2 + (yy - cy) ** 2 < (h / 6.0) ** 2, 230 - tex, y)
        y = np.clip(y, 0, 255).astype(np.uint8)
        u = np.clip(128 + 40 * np.sin((xx[::2, ::2] + 13 * i) / (w / 9.0)), 0, 255).astype(np.uint8)
        v = np.clip(128 - 30 * np.cos((yy[::2, ::2] + 7 * i) / (h / 4.0)), 0, 255).astype(np.uint8)
        uv = np.empty((h // 2, w), np.uint8)
        uv[:, 0::2], uv[:, 1::2] = u, v
        out.append((y, uv))
    return out


def run_stream(E, e, feed, n, oracle=None):
    """submit n pictures through feed(i), collecting whenever three are in flight; with `oracle`, the decode of the whole stream must end in
    the reconstruction the encoder kept (fetched once nothing is in flight any more)"""
    aus = []
    for i in range(n):
        feed(i)
        if e.pending == 3:
            aus.append(e.collect()[0])
    while e.pending:
        aus.append(e.collect()[0])
    if oracle:
        dec = oracle.Decoder()
        for au in aus:
            y, uv = dec.decode(au)
        assert np.array_equal(y, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(uv, e.fetch(E.FETCH_RECON_UV))
    return aus


@pytest.fixture(scope="module")
def scaled_clip(E):
    iw, ih, ow, oh, n = 3840, 2160, 1280, 720, 5
    pics = clip(iw, ih, n)
    ref = [R.to_nv12(R.FMT_NV12, [y, uv], iw, ih, ow, oh) for y, uv in pics]
    enc = E.Encoder(ow, oh, gop=4, fixed_qp=28, pipeline_depth=2)
    aus = run_stream(E, enc, lambda i: enc.submit(ref[i][0][:oh, :ow], ref[i][1][:oh // 2, :ow], pts=i), n)
    enc.close()
    return dict(iw=iw, ih=ih, ow=ow, oh=oh, n=n, pics=pics, aus=aus)


def _scaled_encoder(E, c):
    return E.Encoder(c["ow"], c["oh"], gop=4, fixed_qp=28, pipeline_depth=2, input_size=(c["iw"], c["ih"]))


def test_stream_from_host_nv12_equals_numpy_scaled_stream(E, oracle, scaled_clip):
    c = scaled_clip
    e = _scaled_encoder(E, c)
    aus = run_stream(E, e, lambda i: e.submit(*c["pics"][i], pts=i), c["n"], oracle)
    e.close()
    assert len(aus) == len(c["aus"]) and all(a == b for a, b in zip(aus, c["aus"]))


def test_stream_from_pinned_memory_equals_numpy_scaled_stream(E, scaled_clip):
    c = scaled_clip
    e = _scaled_encoder(E, c)
    iw, ih = c["iw"], c["ih"]
    per = iw * ih * 3 // 2
    buf = E.PinnedBuffer(3 * per)
    views = []
    for k in range(3):
        a = buf.array[k * per:(k + 1) * per]
        views.append((a[:iw * ih].reshape(ih, iw), a[iw * ih:].reshape(ih // 2, iw)))

    def feed(i):
        y, uv = views[i % 3]
        y[:], uv[:] = c["pics"][i]
        e.submit(y, uv, pts=i)
    aus = run_stream(E, e, feed, c["n"])
    assert e.stats().pinned_inputs == c["n"]
    e.close()
    buf.free()
    assert all(a == b for a, b in zip(aus, c["aus"])) and len(aus) == c["n"]


def test_stream_from_device_memory_equals_numpy_scaled_stream(E, scaled_clip):
    """submit_device: the kernel reads the planes where they lie, here at a stride that is not a multiple of 4 and an odd address"""
    c = scaled_clip
    e = _scaled_encoder(E, c)
    iw, ih, stride = c["iw"], c["ih"], c["iw"] + 3
    dev = [device_planes(E, [y, uv], [ih, ih // 2], [iw, iw], stride, 1) for y, uv in c["pics"]]

    def feed(i):
        _, _, (py, puv) = dev[i]
        e.submit_device(py, stride, puv, stride, pts=i)
    aus = run_stream(E, e, feed, c["n"])
    e.close()
    for hip, buf, _ in dev:
        hip.hipFree(buf)
    assert all(a == b for a, b in zip(aus, c["aus"])) and len(aus) == c["n"]


def test_scaled_stream_decodes_to_the_reconstruction_picture_by_picture(E, oracle):
    """pipeline_depth 0: after every picture the oracle decoder's output equals the encoder's reconstruction (an odd ratio with a margin)"""
    iw, ih, ow, oh = 1918, 1078, 642, 362
    e = E.Encoder(ow, oh, gop=3, fixed_qp=26, input_size=(iw, ih))
    dec = oracle.Decoder()
    for i, (y, uv) in enumerate(clip(iw, ih, 4, seed=11)):
        au, _ = e.encode(y, uv, pts=i)
        dy, duv = dec.decode(au)
        assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV)), i
    assert dec.size == (ow, oh)
    e.close()


def test_stream_from_i420_equals_numpy_scaled_stream(E):
    iw, ih, ow, oh, n = 3840, 2160, 1280, 720, 4
    pics = clip(iw, ih, n, seed=9)
    i420 = [[y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])] for y, uv in pics]
    ref = E.Encoder(ow, oh, gop=4, fixed_qp=30, pipeline_depth=2)
    want = []
    for i, p in enumerate(i420):
        ry, ruv = R.to_nv12(R.FMT_I420, p, iw, ih, ow, oh)
        au, _ = ref.encode(ry[:oh, :ow], ruv[:oh // 2, :ow], pts=i)
        want.append(au)
    ref.close()
    e = E.Encoder(ow, oh, gop=4, fixed_qp=30, pipeline_depth=2, input_size=(iw, ih))
    aus = run_stream(E, e, lambda i: e.submit_fmt(E.FMT_I420, i420[i], pts=i), n)
    e.close()
    assert aus == want


def test_input_size_equal_to_the_coded_size_is_the_unscaled_path(E):
    w, h, n = 640, 360, 4
    pics = clip(w, h, n, seed=4)
    a, b = E.Encoder(w, h, gop=4, fixed_qp=27), E.Encoder(w, h, gop=4, fixed_qp=27, input_size=(w, h))
    for i, (y, uv) in enumerate(pics):
        assert a.encode(y, uv, pts=i) == b.encode(y, uv, pts=i), i
    a.close(); b.close()


def test_set_input_size_after_the_first_submit_is_refused(E):
    e = E.Encoder(320, 192, fixed_qp=30)
    y, uv = clip(320, 192, 1)[0]
    e.encode(y, uv)
    assert e.L.mi355enc_set_input_size(e.h, 640, 384) == E.ERR_STATE
    e.close()


def test_set_input_size_refuses_upscaling_large_ratios_and_odd_sizes(E):
    e = E.Encoder(320, 192, fixed_qp=30)
    for w, h in [(318, 192), (320, 190), (2562, 192), (320, 1538), (321, 192), (640, 385)]:
        assert e.L.mi355enc_set_input_size(e.h, w, h) == E.ERR_ARG, (w, h)
    assert e.L.mi355enc_set_input_size(e.h, 2560, 1536) == 0
    e.close()


# ---- the SPS
def sps_of(au):
    """(width in macroblocks, height in macroblocks, aspect_ratio_idc or None, sar) of the SPS that leads an access unit"""
    i = au.index(b"\x00\x00\x01\x67") + 4
    j = au.find(b"\x00\x00\x01", i)
    raw = au[i:j if j > 0 else len(au)]
    rb, k = bytearray(), 0
    while k < len(raw):  # emulation prevention bytes out
        if k + 2 < len(raw) and raw[k] == 0 and raw[k + 1] == 0 and raw[k + 2] == 3:
            rb += b"\x00\x00"; k += 3
        else:
            rb.append(raw[k]); k += 1
    bits = "".join("{:08b}".format(b) for b in rb)
    pos = [0]

    def u(n):
        v = int(bits[pos[0]:pos[0] + n], 2) if n else 0
        pos[0] += n
        return v

    def ue():
        z = 0
        while bits[pos[0]] == "0":
            z += 1; pos[0] += 1
        pos[0] += 1
        return (1 << z) - 1 + u(z)
    profile = u(8); u(8); u(8); ue()
    if profile in (100, 110, 122, 244):
        ue(); ue(); ue(); u(1); assert u(1) == 0
    ue()
    assert ue() == 2  # pic_order_cnt_type
    ue(); u(1)
    mbw, mbh = ue() + 1, ue() + 1
    assert u(1) == 1
    u(1)
    if u(1):
        ue(); ue(); ue(); ue()
    if not u(1):
        return mbw, mbh, None, None
    if not u(1):
        return mbw, mbh, None, None
    idc = u(8)
    return mbw, mbh, idc, (u(16), u(16)) if idc == 255 else None


def test_aspect_changing_scale_writes_the_sar_into_the_vui(E):
    y, uv = clip(1920, 1080, 1)[0]
    e = E.Encoder(1280, 960, fixed_qp=30, input_size=(1920, 1080))
    au, key = e.encode(y, uv)
    e.close()
    assert key and sps_of(au) == (80, 60, 255, (4, 3))


def test_aspect_preserving_scale_keeps_the_headers(E):
    y, uv = clip(3840, 2160, 1)[0]
    e = E.Encoder(1280, 720, fixed_qp=30, input_size=(3840, 2160))
    au, _ = e.encode(y, uv)
    e.close()
    hdr = E.host_write_headers(1280, 720, 60, 1)
    assert au.startswith(hdr) and sps_of(au)[2] is None


# ---- the element
def _run_pipe(tmp_path, name, props, n=6):
    from tests.test_boundary_cpu import HARNESS, gst_env
    from tests.test_gst_gpu import read_records
    pf = tmp_path / ("pipe_" + name)
    pf.write_text("videotestsrc num-buffers=%d ! video/x-raw,width=1920,height=1080,framerate=30/1,format=NV12 ! "
                  "mi355h264enc key-int-max=30 qp=26 %s name=venc_bps ! appsink name=appsink sync=false\n" % (n, props))
    out = tmp_path / ("out_%s.bin" % name)
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return [au for _, au in read_records(str(out))]


def _harness():
    from tests.test_boundary_cpu import HARNESS
    return HARNESS


@pytest.mark.skipif(not os.path.exists(_harness()), reason="oracle/_ref/ref_harness not shipped")
def test_element_scales_to_its_width_and_height(tmp_path, oracle):
    aus = _run_pipe(tmp_path, "scaled", "width=1280 height=720")
    assert len(aus) == 6 and sps_of(aus[0])[:3] == (80, 45, None)
    dec = oracle.Decoder()
    for au in aus:
        y, uv = dec.decode(au)
    assert dec.size == (1280, 720)
    assert float(y[20:300, 5:60].mean()) > 150 and float(y[20:300, 1150:1180].mean()) < 70  # SMPTE bars survive the scale


@pytest.mark.skipif(not os.path.exists(_harness()), reason="oracle/_ref/ref_harness not shipped")
def test_element_width_0_leaves_the_stream(tmp_path):
    assert _run_pipe(tmp_path, "zero", "width=0 height=0", n=3) == _run_pipe(tmp_path, "none", "", n=3)


@pytest.mark.skipif(not os.path.exists(_harness()), reason="oracle/_ref/ref_harness not shipped")
@pytest.mark.parametrize("size,par", [((1280, 720), "1/1"), ((1280, 960), "4/3")])
def test_element_output_caps_carry_the_coded_size(tmp_path, size, par):
    """the caps after the encoder, through a capsfilter that insists on the coded size and on the samples' aspect ratio"""
    from tests.test_boundary_cpu import HARNESS, gst_env
    pf = tmp_path / "pipe_caps"
    pf.write_text("videotestsrc num-buffers=3 ! video/x-raw,width=1920,height=1080,framerate=30/1,format=I420 ! "
                  "mi355h264enc qp=26 width=%d height=%d name=venc_bps ! video/x-h264,width=%d,height=%d,pixel-aspect-ratio=%s ! "
                  "appsink name=appsink sync=false\n" % (size + size + (par,)))
    r = subprocess.run([HARNESS, str(pf), str(tmp_path / "o.bin")], env=gst_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
