"""GPU: automatic levels and white balance inside a GStreamer graph -- the `auto-levels`, `auto-balance`, `auto-speed`, `auto-clip` and `auto-max-gain`
properties of `mi355h264enc`, in the manner of tests/test_adjust_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps
filter, through the project's own probe program, against the C ABI's stream of the same pictures with the corresponding integers."""
import os

import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, nv12_clip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def test_a_launch_line_gives_the_abi_stream_of_the_integers(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    got = _run(tmp_path, "al", blocks, RAW % ("NV12", W, H), "auto-levels=0.9 auto-balance=0.75 auto-speed=64 auto-clip=1.25 auto-max-gain=3.5")
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, autolevel=dict(levels=900, balance=750, speed=64, clip=125, max_gain=3500))
    plain = _abi(E, W, H, col, feed, N)
    assert [g[0] for g in got] != plain
    # the defaults of the three knobs are the library's; both strengths 0: the plain stream, whatever the knobs say
    dflt = _run(tmp_path, "dflt", blocks, RAW % ("NV12", W, H), "auto-levels=1")
    assert [g[0] for g in dflt] == _abi(E, W, H, col, feed, N, autolevel=dict(levels=1000))
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), "auto-levels=0 auto-balance=0 auto-speed=256 auto-clip=5 auto-max-gain=8")
    assert [g[0] for g in off] == plain


def test_a_property_written_in_playing_takes_effect_on_the_next_picture(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "auto-balance=0.5", args=("--set", "2", "auto-levels", "1"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_autolevel(balance=500, levels=1000)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60, autolevel=dict(balance=500))
    still = _run(tmp_path, "still", blocks, RAW % ("NV12", W, H), "auto-balance=0.5", gop=60)
    assert [g[0] for g in still[:2]] == [g[0] for g in got[:2]] and still[2][0] != got[2][0]
