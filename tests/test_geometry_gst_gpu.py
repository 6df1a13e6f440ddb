"""GPU: the input geometry inside a GStreamer graph -- `mi355h264enc`'s crop-left/right/top/bottom, add-borders, upscale and border-color,
in the manner of tests/test_orient_gst_gpu.py, driven through the project's own probe program: the element's stream is the C ABI's for the same geometry."""
import os

import numpy as np
import pytest

from tests import geomref as G
from tests import orientref as R
from tests.spsref import nal_units, sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gpu import JPEG, clips
from tests.test_orient_gst_gpu import RAW, _abi, _raw, _run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, N = 208, 120, 5


def test_add_borders_with_90r_pillarboxes_the_turned_picture(tmp_path, E, oracle):
    """a 208 x 120 picture turned by 90r stands 120 x 208; add-borders places it, 70 x 120, in the 208 x 120 programme"""
    pics, _ = clips(H, W, 1)  # (pre-orientation pictures of 208 x 120)
    assert pics[0][0].shape == (H, W)
    got = _run(tmp_path, "pillar", _raw(pics), RAW % (W, H), "video-direction=90r add-borders=true width=%d height=%d" % (W, H))
    assert all((w, h) == (W, H) for _, w, h in got)  # the source caps: the programme's size
    (s,) = sps_of(got[0][0])
    assert (s["mbw"], s["mbh"]) == ((W + 15) // 16, (H + 15) // 16) and s["sar"] is None
    dst = G.fit_rect(W, H, H, W)  # the geometry works in front of the orientation: the target is 120 x 208
    assert dst == (0, 68, 120, 70) and E.fit_rect(W, H, H, W) == dst
    g = E.geometry((W, H), dst=dst, keep_sar=True)
    abi = _abi(E, W, H, s["colorimetry"], lambda e, i: e.submit(*pics[i], pts=i), N, orientation="90r", geometry=g)
    assert [a for a, _, _ in got] == abi
    # decodable, and the first picture's border columns are the border colour within coding error
    dec = oracle.Decoder()
    dy, duv = dec.decode(got[0][0])
    for au, _, _ in got[1:]:
        dec.decode(au)
    my, _ = R.orient(np.pad(np.ones((70, 120), np.uint8), ((68, 70), (0, 0))), np.zeros((104, 120), np.uint8), 1)  # 1 inside the destination rectangle, turned
    assert my.shape == (H, W) and int(my.sum()) == 70 * 120 and (my[:, :68] == 0).all() and (my[:, 140:] == 0).all()  # (a pillar 70 wide, borders of 68 and 70)
    border = dy[:H, :W][my == 0].astype(np.int64)
    assert abs(border.mean() - 16) <= 3 and np.abs(border - 16).max() <= 24
    chroma = duv[:H // 2, :68].astype(np.int64)
    assert abs(chroma.mean() - 128) <= 3


def test_crop_set_in_mid_stream_takes_effect_without_new_caps(tmp_path, E):
    """crop-left / -right in front of picture 2, with add-borders (the shape of the crop may then change): the handle takes it through mi355enc_set_crop -- no
    drain, no parameter sets, no new caps -- and the stream is the C ABI's with the same call in front of the same picture"""
    pics, _ = clips(W, H, 0)
    props = "add-borders=true width=%d height=%d crop-top=2" % (W, H - 2)
    got = _run(tmp_path, "recrop", _raw(pics), RAW % (W, H), props, args=("--set", "2", "crop-left", "41"), gop=60)
    assert [(w, h) for _, w, h in got] == [(W, H - 2)] * N
    types = [[t for t, _, _ in nal_units(au)] for au, _, _ in got]
    assert 7 in types[0] and all(7 not in t and 5 not in t for t in types[1:])
    (s,) = sps_of(got[0][0])

    def feed(e, i):
        if i == 2:
            e.set_crop(40, 2, W - 40, H - 2)  # (41 counts as 40)
        e.submit(*pics[i], pts=i)
    g = E.geometry((W, H), crop=(0, 2, W, H - 2), target=(W, H - 2), keep_sar=True)
    assert [a for a, _, _ in got] == _abi(E, W, H - 2, s["colorimetry"], feed, N, gop=60, geometry=g)
    still = _run(tmp_path, "still", _raw(pics), RAW % (W, H), props, gop=60)
    assert [a for a, _, _ in still[:2]] == [a for a, _, _ in got[:2]] and still[2][0] != got[2][0]
    # without add-borders a crop of another shape is a new stream: drained and reopened, as after a caps change
    got = _run(tmp_path, "reopen", _raw(pics), RAW % (W, H), "upscale=true width=%d height=%d crop-top=2" % (W, H - 2), args=("--set", "2", "crop-left", "40"), gop=60)
    types = [[t for t, _, _ in nal_units(au)] for au, _, _ in got]
    assert 7 in types[2] and 5 in types[2] and sps_of(got[2][0])[0]["sar"] is not None and sps_of(got[0][0])[0]["sar"] is None


def test_upscaled_jpeg_with_borders(tmp_path, E):
    """the webcam shape: a 72 x 40 MJPEG picture into 128 x 96 with borders, behind the in-encoder decode"""
    data = open(JPEG, "rb").read()
    caps = "image/jpeg,width=72,height=40,framerate=30/1"
    got = _run(tmp_path, "up", [data] * N, caps, "add-borders=true upscale=true width=128 height=96 border-color=0x306090")
    assert all((w, h) == (128, 96) for _, w, h in got)
    dst = G.fit_rect(72, 40, 128, 96)
    g = E.geometry((72, 40), dst=dst, keep_sar=True, border=(0x30, 0x60, 0x90))
    assert [a for a, _, _ in got] == _abi(E, 128, 96, (1, 2, 2, 6), lambda e, i: e.submit_jpeg(data, pts=i), N, geometry=g)


def test_every_new_property_at_its_default_changes_nothing(tmp_path):
    pics, _ = clips(W, H, 0)
    defaults = "crop-left=0 crop-right=0 crop-top=0 crop-bottom=0 add-borders=false upscale=false border-color=0x108080"
    for props in ("", "width=104 height=60", "video-direction=90r"):
        assert _run(tmp_path, "with", _raw(pics), RAW % (W, H), props + " " + defaults) == _run(tmp_path, "without", _raw(pics), RAW % (W, H), props)
