"""GPU: temporal noise reduction inside a GStreamer graph -- the `denoise-luma` and `denoise-chroma` properties of `mi355h264enc`, in the
manner of tests/test_adjust_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through the project's own probe program, against
the C ABI's stream of the same pictures with the same strengths."""
import os

import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_denoise_gpu import noisy_clip
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def test_a_launch_line_gives_the_abi_stream_of_the_same_strengths(tmp_path, E):
    pics = noisy_clip(W, H, N, 31)
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    got = _run(tmp_path, "dn", blocks, RAW % ("NV12", W, H), "denoise-luma=8 denoise-chroma=8")
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, denoise=dict(luma=8, chroma=8))
    plain = _abi(E, W, H, col, feed, N)
    assert got[0][0] == plain[0] and [g[0] for g in got[1:]] != plain[1:]  # (the first picture primes)
    luma = _run(tmp_path, "luma", blocks, RAW % ("NV12", W, H), "denoise-luma=16")
    assert [g[0] for g in luma] == _abi(E, W, H, col, feed, N, denoise=dict(luma=16))
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), "denoise-luma=0 denoise-chroma=0")
    assert [g[0] for g in off] == plain


def test_a_property_written_in_playing_takes_effect_on_a_later_picture(tmp_path, E):
    pics = noisy_clip(W, H, N, 32)
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "denoise-luma=4", args=("--set", "2", "denoise-luma", "16"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_denoise(luma=16)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60, denoise=dict(luma=4))
    still = _run(tmp_path, "still", blocks, RAW % ("NV12", W, H), "denoise-luma=4", gop=60)
    assert [g[0] for g in still[:2]] == [g[0] for g in got[:2]] and still[2][0] != got[2][0]
