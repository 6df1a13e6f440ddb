"""GPU: the colour step and the 10-bit / grey formats inside a GStreamer graph -- the `output-colorimetry` property of `mi355h264enc` and its new sink caps
(DESIGN.md section 20), in the manner of tests/test_orient_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through the
project's own probe program, against the C ABI's stream of the same pictures."""
import os
import subprocess

import numpy as np
import pytest

from ceracoder_amd import synth
from tests import yuvref as R
from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE, gst_env
from tests.test_orient_gst_gpu import _abi, _run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, N = 320, 180, 5
RAW = "video/x-raw,format=%s,width=%d,height=%d,framerate=30/1"


def nv12_clip():
    return [(np.ascontiguousarray(y[:H, :W]), np.ascontiguousarray(uv[:H // 2, :W])) for y, uv in synth.s2_frames(W, H, N)]


def test_output_colorimetry_converts_bt601_input_to_bt709(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    caps = RAW % ("NV12", W, H) + ",colorimetry=(string)bt601"
    got = _run(tmp_path, "conv", blocks, caps, "output-colorimetry=bt709")
    (s,) = sps_of(got[0][0])
    assert s["colorimetry"] == (0, 1, 1, 1)
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, (0, 1, 1, 1), feed, N, input_colorimetry=(0, 6))
    # (c) without the property: labelled as the input, nothing converted -- today's stream
    plain = _run(tmp_path, "plain", blocks, caps, "")
    assert sps_of(plain[0][0])[0]["colorimetry"] == (0, 6, 6, 6)
    assert [g[0] for g in plain] == _abi(E, W, H, (0, 6, 6, 6), feed, N)
    assert [g[0] for g in plain] != [g[0] for g in got]
    # ... and with the property naming what the input already is: the same pictures
    same = _run(tmp_path, "same", blocks, caps, "output-colorimetry=bt601")
    assert [g[0] for g in same] == [g[0] for g in plain]


def gst_frame(fmt, rng):
    """one 320 x 180 picture in GStreamer's layout of the format -> (the buffer's bytes, the planes as the library is handed them)"""
    if fmt == R.FMT_P010:  # strides 640, 640
        buf = rng.integers(0, 256, 640 * H + 640 * H // 2, dtype=np.uint8)
        return buf, [buf[:640 * H].reshape(H, 640), buf[640 * H:].reshape(H // 2, 640)]
    if fmt == R.FMT_I420_10:  # strides 640, 320, 320
        buf = rng.integers(0, 256, 640 * H + 2 * 320 * H // 2, dtype=np.uint8)
        o1, o2 = 640 * H, 640 * H + 320 * H // 2
        return buf, [buf[:o1].reshape(H, 640), buf[o1:o2].reshape(H // 2, 320), buf[o2:].reshape(H // 2, 320)]
    if fmt == R.FMT_V210:  # stride ((w + 47) / 48) 128 = 896, of which a row reads ceil(w / 6) 16 = 864
        buf = rng.integers(0, 256, 896 * H, dtype=np.uint8)
        return buf, [buf.reshape(H, 896)]
    buf = rng.integers(0, 256, W * H, dtype=np.uint8)  # GRAY8: stride 320
    return buf, [buf.reshape(H, W)]


@pytest.mark.parametrize("fmt,name", [(R.FMT_P010, "P010_10LE"), (R.FMT_I420_10, "I420_10LE"), (R.FMT_V210, "v210"), (R.FMT_GRAY8, "GRAY8")], ids=["P010", "I420_10", "v210", "GRAY8"])
def test_element_takes_the_deep_formats_without_videoconvert(tmp_path, E, fmt, name):
    rng = np.random.default_rng(fmt)
    frames = [gst_frame(fmt, rng) for _ in range(N)]
    got = _run(tmp_path, name, [f[0].tobytes() for f in frames], RAW % (name, W, H), "")
    (s,) = sps_of(got[0][0])
    abi = _abi(E, W, H, s["colorimetry"], lambda e, i: e.submit_fmt(fmt, frames[i][1], pts=i), N)
    assert [g[0] for g in got] == abi
    # ... which is the stream of the pictures tests/yuvref.py makes of them
    conv = [R.to_nv12(fmt, f[1], W, H) for f in frames]
    assert abi == _abi(E, W, H, s["colorimetry"], lambda e, i: e.submit(conv[i][0][:H, :W], conv[i][1][:H // 2, :W], pts=i), N)


def test_an_output_colorimetry_that_does_not_parse_fails_through_the_bus(tmp_path):
    y, uv = nv12_clip()[0]
    src = tmp_path / "one.src"
    src.write_bytes(y.tobytes() + uv.tobytes())
    for value, what in (("nonsense", "is not a colorimetry"), ("2:2:0:0", "cannot open")):  # (2:2:0:0: limited range, matrix FCC -- a conversion the library refuses)
        desc = "filesrc location=%s blocksize=%d ! %s ! mi355h264enc qp=28 output-colorimetry=%s name=venc_bps ! appsink name=appsink sync=false" % (
            src, W * H * 3 // 2, RAW % ("NV12", W, H), value)
        r = subprocess.run([PROBE, desc], env=gst_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "gstreamer error" in r.stderr and what in r.stderr, r.stderr[-2000:]
