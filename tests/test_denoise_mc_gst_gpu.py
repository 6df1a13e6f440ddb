"""GPU: the `denoise-motion` property of `mi355h264enc` inside a GStreamer graph, in the manner of tests/test_denoise_gst_gpu.py: set at
the start, changed in PLAYING, refused outside its range, each time against the C ABI's stream of the same pictures with the same settings."""
import os

import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_denoise_mc_gpu import moving_clip
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def test_a_launch_line_gives_the_abi_stream_of_the_same_range(tmp_path, E):
    pics = moving_clip(W, H, N, 51)
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    got = _run(tmp_path, "mc", blocks, RAW % ("NV12", W, H), "denoise-luma=8 denoise-chroma=8 denoise-motion=8")
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, denoise=dict(luma=8, chroma=8, motion=8))
    plain = _abi(E, W, H, col, feed, N, denoise=dict(luma=8, chroma=8))
    assert [g[0] for g in got[:1]] == plain[:1] and [g[0] for g in got[1:]] != plain[1:]  # (the first picture primes; from the second on the search runs)
    # a range without strengths is off
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), "denoise-motion=16")
    assert [g[0] for g in off] == _abi(E, W, H, col, feed, N)


def test_the_range_written_in_playing_takes_effect_on_a_later_picture_and_one_outside_is_refused(tmp_path, E):
    pics = moving_clip(W, H, N, 52, step=(7, -6))  # (out of reach at range 4, within it at 16)
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "denoise-luma=8 denoise-motion=4", args=("--set", "2", "denoise-motion", "16"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_denoise_motion(16)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60, denoise=dict(luma=8, motion=4))
    still = _run(tmp_path, "still", blocks, RAW % ("NV12", W, H), "denoise-luma=8 denoise-motion=4", gop=60)
    assert [g[0] for g in still[:2]] == [g[0] for g in got[:2]] and [g[0] for g in still[2:]] != [g[0] for g in got[2:]]
    # 17 is outside the property's range: GObject refuses the write, the element keeps 4
    bad = _run(tmp_path, "bad", blocks, RAW % ("NV12", W, H), "denoise-luma=8 denoise-motion=4", args=("--set", "2", "denoise-motion", "17"), gop=60)
    assert [g[0] for g in bad] == [g[0] for g in still]
