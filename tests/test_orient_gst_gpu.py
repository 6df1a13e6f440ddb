"""GPU: orientation inside a GStreamer graph -- the `video-direction` property of `mi355h264enc` (the GstVideoDirection interface, as on `videoflip`), its
`auto` mode behind an image-orientation tag, a change of direction while running, and MJPEG caps; in the manner of tests/test_overlay_gst_gpu.py, driven
through the project's own probe program, which can report the source caps' size, send a tag and set a property in mid-stream."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import orientref as R
from tests.spsref import nal_units, sps_of
from tests.test_boundary_cpu import PROBE, gst_env
from tests.test_orient_gpu import JPEG, clips

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, QP, N = 208, 120, 28, 5
RAW = "video/x-raw,format=NV12,width=%d,height=%d,framerate=30/1"


def _run(tmp_path, name, blocks, caps, props, args=(), gop=4):
    """-> [(access unit, width, height of the source caps)]"""
    src, out = tmp_path / (name + ".src"), tmp_path / (name + ".bin")
    size = max(len(b) for b in blocks)
    src.write_bytes(b"".join(b + bytes(size - len(b)) for b in blocks))
    desc = "filesrc location=%s blocksize=%d ! %s ! mi355h264enc qp=%d key-int-max=%d %s name=venc_bps ! appsink name=appsink sync=false" % (src, size, caps, QP, gop, props)
    r = subprocess.run([PROBE, desc, "--dump", str(out)] + list(args), env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data, recs, o = out.read_bytes(), [], 0
    while o < len(data):  # records {u32 length, u32 width, u32 height, bytes}
        n, w, h = struct.unpack_from("<III", data, o)
        recs.append((data[o + 12:o + 12 + n], w, h))
        o += 12 + n
    assert len(recs) == len(blocks)
    return recs


def _raw(pics):
    return [y.tobytes() + uv.tobytes() for y, uv in pics]


def _abi(E, w, h, colorimetry, feed, n, gop=4, **kw):
    """the C ABI's access units for the same stream settings the element opens with"""
    e = E.Encoder(w, h, fps=30, gop=gop, fixed_qp=QP, colorimetry=colorimetry, slices=None, slice_deblock=None, **kw)
    out = []
    for i in range(n):
        feed(e, i)
        out.append(e.collect()[0])
    e.close()
    return out


def test_direction_90r_exchanges_the_caps_and_gives_the_abi_stream_of_the_turned_pictures(tmp_path, E):
    pics, oriented = clips(H, W, 1)  # coded 120 x 208 from 208 x 120 input
    assert pics[0][0].shape == (H, W) and oriented[0][0].shape == (W, H)
    got = _run(tmp_path, "r90", _raw(pics), RAW % (W, H), "video-direction=90r")
    assert all((w, h) == (H, W) for _, w, h in got)
    (s,) = sps_of(got[0][0])
    assert (s["mbw"], s["mbh"]) == ((H + 15) // 16, (W + 15) // 16)
    abi = _abi(E, H, W, s["colorimetry"], lambda e, i: e.submit(*oriented[i], pts=i), N)
    assert [g[0] for g in got] == abi
    # ... which is also the element's own stream of the pre-oriented pictures, and the C ABI's with the orientation done on the device
    plain = _run(tmp_path, "pre", _raw(oriented), RAW % (H, W), "")
    assert [g[0] for g in plain] == abi and all((w, h) == (H, W) for _, w, h in plain)
    assert _abi(E, H, W, s["colorimetry"], lambda e, i: e.submit(*pics[i], pts=i), N, orientation="90r") == abi


def test_auto_follows_the_image_orientation_tag(tmp_path):
    pics, _ = clips(W, H, 2)
    by_tag = _run(tmp_path, "auto", _raw(pics), RAW % (W, H), "video-direction=auto", args=("--tag", "rotate-180"))
    by_prop = _run(tmp_path, "p180", _raw(pics), RAW % (W, H), "video-direction=180")
    ident = _run(tmp_path, "ident", _raw(pics), RAW % (W, H), "video-direction=identity", args=("--tag", "rotate-180"))  # (not auto: the tag is not followed)
    assert by_tag == by_prop
    assert by_tag[0][0] != ident[0][0]
    # a transposing tag exchanges the caps as the property does
    flip = _run(tmp_path, "auto90", _raw(pics), RAW % (W, H), "video-direction=auto", args=("--tag", "rotate-90"))
    assert flip == _run(tmp_path, "p90", _raw(pics), RAW % (W, H), "video-direction=90r") and flip[0][1:] == (H, W)


def test_a_direction_set_while_running_starts_a_new_stream_at_the_new_size(tmp_path, E):
    """identity -> 90l in front of picture 3 (key-int-max 60: no IDR picture is due there): the encoder is drained and reopened, picture 3 is an IDR picture
    behind new parameter sets of 120 x 208, and from there on the stream is that of a fresh encoder fed the turned pictures"""
    pics, _ = clips(W, H, 0)
    got = _run(tmp_path, "switch", _raw(pics), RAW % (W, H), "video-direction=identity", args=("--set", "3", "video-direction", "90l"), gop=60)
    assert [(w, h) for _, w, h in got] == [(W, H)] * 3 + [(H, W)] * 2
    types = [[t for t, _, _ in nal_units(au)] for au, _, _ in got]
    assert 7 in types[0] and 5 in types[0] and all(7 not in t and 5 not in t for t in types[1:3])
    assert 7 in types[3] and 8 in types[3] and 5 in types[3] and 5 not in types[4]
    (s,) = sps_of(got[3][0])
    assert (s["mbw"], s["mbh"]) == ((H + 15) // 16, (W + 15) // 16)
    turned = [R.orient(y, uv, 3) for y, uv in pics[3:]]
    assert [g[0] for g in got[3:]] == _abi(E, H, W, s["colorimetry"], lambda e, i: e.submit(*turned[i], pts=i), 2, gop=60)
    (s0,) = sps_of(got[0][0])
    assert [g[0] for g in got[:3]] == _abi(E, W, H, s0["colorimetry"], lambda e, i: e.submit(*pics[i], pts=i), 3, gop=60)


def test_jpeg_caps_with_a_direction_give_the_abi_jpeg_stream(tmp_path, E):
    data = open(JPEG, "rb").read()
    got = _run(tmp_path, "jpeg", [data] * N, "image/jpeg,width=72,height=40,framerate=30/1", "video-direction=horiz")
    assert all((w, h) == (72, 40) for _, w, h in got)
    abi = _abi(E, 72, 40, (1, 2, 2, 6), lambda e, i: e.submit_jpeg(data, pts=i), N, orientation="horiz")
    assert [g[0] for g in got] == abi
    # ... and turned: the source caps carry the exchanged size
    got = _run(tmp_path, "jpeg90", [data] * N, "image/jpeg,width=72,height=40,framerate=30/1", "video-direction=90r")
    assert all((w, h) == (40, 72) for _, w, h in got)
    assert [g[0] for g in got] == _abi(E, 40, 72, (1, 2, 2, 6), lambda e, i: e.submit_jpeg(data, pts=i), N, orientation="90r")
