"""GPU: the privacy masks inside a GStreamer graph -- the `mask` and `mask-color` properties of `mi355h264enc`, in the manner of
tests/test_roi_gst_gpu.py: known frames from `filesrc blocksize=<frame>` behind a caps filter, through the project's own probe program, against the C ABI's
stream of the same pictures with the configuration mi355enc_mask_parse reads from the same string."""
import os

import pytest

from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import _abi, _run
from tests.test_yuv_convert_gst_gpu import H, N, RAW, W, nv12_clip

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

TEXT = "80,48,128,80,3,9,1;-16,100,64,200,2,12;200,20,60,40,1,0"
COLOUR = 0x30A0E0


def with_mask(E, pics, text, colour, at=0):
    def feed(e, i):
        if i == at:
            e.set_mask(E.mask_parse(text, colour))
        e.submit(*pics[i], pts=i)
    return feed


def plain(pics):
    return lambda e, i: e.submit(*pics[i], pts=i)


def test_a_launch_line_with_masks_gives_the_abis_bytes(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "mask", blocks, RAW % ("NV12", W, H), 'mask="%s" mask-color=%d' % (TEXT, COLOUR))
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, with_mask(E, pics, TEXT, COLOUR), N)
    assert got[0][0] != _abi(E, W, H, col, plain(pics), N)[0] and got[0][0] != _abi(E, W, H, col, with_mask(E, pics, TEXT, 0), N)[0]
    # an empty string: the plain stream
    off = _run(tmp_path, "off", blocks, RAW % ("NV12", W, H), 'mask="" mask-color=%d' % COLOUR)
    assert [g[0] for g in off] == _abi(E, W, H, col, plain(pics), N)


def test_masks_written_in_playing_take_effect_from_a_later_frame_on(tmp_path, E):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    late = _run(tmp_path, "late", blocks, RAW % ("NV12", W, H), "", args=("--set", "2", "mask", TEXT), gop=60)
    col = sps_of(late[0][0])[0]["colorimetry"]
    assert [g[0] for g in late] == _abi(E, W, H, col, with_mask(E, pics, TEXT, 0, at=2), N, gop=60)
    assert late[2][0] != _abi(E, W, H, col, plain(pics), N, gop=60)[2]


@pytest.mark.parametrize("on", [False, True], ids=["while-off", "while-on"])
def test_a_junk_string_warns_and_leaves_a_running_stream_as_it_was(tmp_path, E, on):
    pics = nv12_clip()
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    got = _run(tmp_path, "bad", blocks, RAW % ("NV12", W, H), 'mask="%s"' % TEXT if on else "", args=("--set", "2", "mask", "80,48,128,80,3,33"), gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]
    assert [g[0] for g in got] == _abi(E, W, H, col, with_mask(E, pics, TEXT, 0) if on else plain(pics), N, gop=60)  # every picture there, coded as before the write
