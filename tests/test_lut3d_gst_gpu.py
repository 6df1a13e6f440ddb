"""GPU: the 3D colour LUT inside a GStreamer graph -- the `lut3d-location` and `lut3d-strength` properties of `mi355h264enc`, in the manner
of tests/test_autolevel_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through the project's own probe program, against the C
ABI's stream of the same pictures with the table the reference's parser reads from the same file."""
import os

import pytest

from tests import lut3dref as R
from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_lut3d_cpu import GOLDEN
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, nv12_clip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]


def with_lut(pics, nodes, strength=256):
    def feed(e, i):
        if i == 0:
            e.set_lut3d(nodes, strength)
        e.submit(*pics[i], pts=i)
    return feed


@pytest.mark.parametrize("props,strength", [("", 256), (" lut3d-strength=0.5", 128), (" lut3d-strength=0", 0)], ids=["full", "half", "zero"])
def test_a_launch_line_with_the_golden_file_gives_the_mirrors_bytes(tmp_path, E, props, strength):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    nodes, size = R.parse_cube(open(GOLDEN, "rb").read())
    got = _run(tmp_path, "lut", blocks, RAW % ("NV12", W, H), "lut3d-location=%s%s" % (GOLDEN, props))
    col = sps_of(got[0][0])[0]["colorimetry"]
    plain = _abi(E, W, H, col, lambda e, i: e.submit(*pics[i], pts=i), N)
    assert [g[0] for g in got] == _abi(E, W, H, col, with_lut(pics, nodes, strength), N)
    assert ([g[0] for g in got] == plain) == (strength == 0)


def test_a_location_written_in_playing_takes_effect_on_the_next_picture(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    nodes, size = R.parse_cube(open(GOLDEN, "rb").read())
    late = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "", args=("--set", "2", "lut3d-location", GOLDEN), gop=60)
    col = sps_of(late[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 2:
            e.set_lut3d(nodes)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in late] == _abi(E, W, H, col, feed, N, gop=60)
    assert late[2][0] != _abi(E, W, H, col, lambda e, i: e.submit(*pics[i], pts=i), N, gop=60)[2]


@pytest.mark.parametrize("kind", ["missing", "refused", "missing-while-on"])
def test_a_bad_path_leaves_a_running_stream_running_and_as_it_was(tmp_path, E, kind):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    bad = tmp_path / "bad.cube"
    if kind == "refused":
        bad.write_text("LUT_1D_SIZE 2\n0 0 0\n1 1 1\n")
    nodes, _ = R.parse_cube(open(GOLDEN, "rb").read())
    on = kind == "missing-while-on"
    got = _run(tmp_path, "bad", blocks, RAW % ("NV12", W, H), "lut3d-location=%s" % GOLDEN if on else "", args=("--set", "2", "lut3d-location", str(bad)), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]
    feed = with_lut(pics, nodes) if on else (lambda e, i: e.submit(*pics[i], pts=i))
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60)  # every picture there, graded as before the write
