"""GPU: the spatial noise filter inside a GStreamer graph -- the `denoise-spatial-luma`, `denoise-spatial-chroma`, `denoise-auto`, `denoise-auto-percentile` and
`denoise-auto-speed` properties of `mi355h264enc`, in the manner of tests/test_lut3d_gst_gpu.py: known frames from
`filesrc blocksize=<frame>` behind a caps filter, through the project's own probe program, against the C ABI's stream of the same pictures with the corresponding
integers."""
import os

import numpy as np
import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, nv12_clip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def noisy_clip():
    """the synthetic clip with Gaussian noise of 3 codes on every sample"""
    rng = np.random.default_rng(30)
    add = lambda p: np.clip(np.rint(p + 3.0 * rng.standard_normal(p.shape)), 0, 255).astype(np.uint8)
    return [(add(y), add(uv)) for y, uv in nv12_clip()]


def test_a_launch_line_gives_the_abi_stream_of_the_integers(tmp_path, E):
    pics = noisy_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    feed = lambda e, i: e.submit(*pics[i], pts=i)
    got = _run(tmp_path, "manual", blocks, RAW % ("NV12", W, H), "denoise-spatial-luma=8 denoise-spatial-chroma=6")
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, denoise_spatial=dict(luma=8, chroma=6))
    plain = _abi(E, W, H, col, feed, N)
    assert [g[0] for g in got] != plain
    auto = _run(tmp_path, "auto", blocks, RAW % ("NV12", W, H), "denoise-spatial-luma=16 denoise-spatial-chroma=12 denoise-auto=2.5 denoise-auto-percentile=40 denoise-auto-speed=200")
    want = _abi(E, W, H, col, feed, N, denoise_spatial=dict(luma=16, chroma=12, auto_gain=2500, percentile=40, speed=200))
    assert [g[0] for g in auto] == want and want != plain and want != [g[0] for g in got]
    # the defaults of the two knobs are the library's; nothing that filters or measures: the plain stream, whatever the knobs say
    dflt = _run(tmp_path, "dflt", blocks, RAW % ("NV12", W, H), "denoise-spatial-luma=16 denoise-auto=2")
    assert [g[0] for g in dflt] == _abi(E, W, H, col, feed, N, denoise_spatial=dict(luma=16, auto_gain=2000))
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), "denoise-spatial-luma=0 denoise-spatial-chroma=0 denoise-auto=0 denoise-auto-percentile=50 denoise-auto-speed=256")
    assert [g[0] for g in off] == plain


def test_a_property_written_in_playing_takes_effect_on_the_next_picture(tmp_path, E):
    pics = noisy_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "denoise-spatial-chroma=5", args=("--set", "2", "denoise-spatial-luma", "9"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_denoise_spatial(chroma=5, luma=9)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60, denoise_spatial=dict(chroma=5))
    still = _run(tmp_path, "still", blocks, RAW % ("NV12", W, H), "denoise-spatial-chroma=5", gop=60)
    assert [g[0] for g in still[:2]] == [g[0] for g in got[:2]] and still[2][0] != got[2][0]
