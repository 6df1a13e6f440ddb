"""GPU: HDR input inside a GStreamer graph -- the `hdr-input`, `hdr-peak-nits` and `hdr-target-nits` properties of `mi355h264enc`, in the
manner of tests/test_yuv_convert_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through the project's own probe program,
against the C ABI's stream of the same pictures."""
import os
import subprocess

import numpy as np
import pytest

from tests import yuvref as R
from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE, gst_env
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, gst_frame

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

PQ = 16


@pytest.mark.parametrize("fmt,name", [(R.FMT_P010, "P010_10LE"), (R.FMT_V210, "v210")], ids=["P010", "v210"])
def test_hdr_input_pq_equals_the_abi_stream_and_says_bt709(tmp_path, E, fmt, name):
    rng = np.random.default_rng(fmt)
    frames = [gst_frame(fmt, rng) for _ in range(N)]
    blocks = [f[0].tobytes() for f in frames]
    caps = RAW % (name, W, H) + ",colorimetry=(string)bt2020"
    feed = lambda e, i: e.submit_fmt(fmt, frames[i][1], pts=i)
    got = _run(tmp_path, name, blocks, caps, "hdr-input=pq")
    assert sps_of(got[0][0])[0]["colorimetry"] == (0, 1, 1, 1)  # never the caps' bt2020 label
    assert [g[0] for g in got] == _abi(E, W, H, (0, 1, 1, 1), feed, N, hdr_input=(PQ, 0, 0, 0))
    # ... with an output colorimetry: that one, and other pictures
    got601 = _run(tmp_path, name + "601", blocks, caps, "hdr-input=pq output-colorimetry=bt601")
    assert sps_of(got601[0][0])[0]["colorimetry"] == (0, 6, 6, 6)
    assert [g[0] for g in got601] == _abi(E, W, H, (0, 6, 6, 6), feed, N, hdr_input=(PQ, 0, 0, 0))
    assert [g[0] for g in got601] != [g[0] for g in got]
    if fmt == R.FMT_P010:  # the peak and the target reach the setter
        dim = _run(tmp_path, name + "dim", blocks, caps, "hdr-input=pq hdr-peak-nits=4000 hdr-target-nits=100")
        assert [g[0] for g in dim] == _abi(E, W, H, (0, 1, 1, 1), feed, N, hdr_input=(PQ, 0, 4000, 100))
        assert [g[0] for g in dim] != [g[0] for g in got]


def test_hdr_input_on_8_bit_caps_fails_through_the_bus(tmp_path):
    src = tmp_path / "one.src"
    src.write_bytes(bytes(W * H * 3 // 2))
    desc = "filesrc location=%s blocksize=%d ! %s ! mi355h264enc qp=28 hdr-input=hlg name=venc_bps ! appsink name=appsink sync=false" % (src, W * H * 3 // 2, RAW % ("NV12", W, H))
    r = subprocess.run([PROBE, desc], env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "gstreamer error" in r.stderr and "hdr-input needs" in r.stderr, r.stderr[-2000:]
