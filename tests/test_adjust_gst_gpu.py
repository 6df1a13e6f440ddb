"""GPU: picture controls inside a GStreamer graph -- the `brightness`, `contrast`, `hue`, `saturation`, `gamma`, `sharpen` and `sharpen-threshold` properties of
`mi355h264enc`, in the manner of tests/test_hdr_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through
the project's own probe program, against the C ABI's stream of the same pictures with the corresponding thousandths."""
import os

import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, nv12_clip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def test_a_launch_line_gives_the_abi_stream_of_the_thousandths(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    got = _run(tmp_path, "adj", blocks, RAW % ("NV12", W, H), "brightness=0.1 contrast=1.2 saturation=0.8 sharpen=16")
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, adjust=dict(brightness=100, contrast=1200, saturation=800, sharpen=16))
    plain = _abi(E, W, H, col, feed, N)
    assert [g[0] for g in got] != plain
    # the other three reach the setter too; all at their defaults: the plain stream
    more = _run(tmp_path, "more", blocks, RAW % ("NV12", W, H), "hue=-0.25 gamma=2.2 sharpen=24 sharpen-threshold=4")
    assert [g[0] for g in more] == _abi(E, W, H, col, feed, N, adjust=dict(hue=-250, gamma=2200, sharpen=24, sharpen_threshold=4))
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), "brightness=0 contrast=1 hue=0 saturation=1 gamma=1 sharpen=0 sharpen-threshold=8")
    assert [g[0] for g in off] == plain


def test_a_property_written_in_playing_takes_effect_on_a_later_picture(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "contrast=1.1", args=("--set", "2", "sharpen", "32"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_adjust(contrast=1100, sharpen=32)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60, adjust=dict(contrast=1100))
    still = _run(tmp_path, "still", blocks, RAW % ("NV12", W, H), "contrast=1.1", gop=60)
    assert [g[0] for g in still[:2]] == [g[0] for g in got[:2]] and still[2][0] != got[2][0]
