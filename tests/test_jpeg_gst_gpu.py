"""GPU: MJPEG input inside a GStreamer graph -- `image/jpeg` caps on the sink pad of `mi355h264enc`, driven like tests/test_overlay_gst_gpu.py.
The pipeline loader takes a pipeline that feeds itself, so the pictures come from `filesrc` in blocks of one size: every JPEG picture is padded
behind its EOI marker to the longest one's length (a decoder stops at the end of the scan)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import jpegref as J
from tests.spsref import sps_of
from tests.test_boundary_cpu import HARNESS, gst_env

pytestmark = pytest.mark.gpu

W, H, QP, N = 64, 48, 28, 6
ENC = "mi355h264enc qp=%d key-int-max=4 name=venc_bps ! appsink name=appsink sync=false\n" % QP


def _run(tmp_path, name, blocks, caps, want):
    src, pf, out = tmp_path / (name + ".src"), tmp_path / name, tmp_path / (name + ".bin")
    size = max(len(b) for b in blocks)
    src.write_bytes(b"".join(b + bytes(size - len(b)) for b in blocks))
    pf.write_text("filesrc location=%s blocksize=%d ! %s ! %s" % (src, size, caps, ENC))
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data, aus, o = out.read_bytes(), [], 0
    while o < len(data):  # records {u32 length, u64 pts_ns, bytes}
        n, _ = struct.unpack_from("<IQ", data, o)
        aus.append(data[o + 12:o + 12 + n])
        o += 12 + n
    assert len(aus) == want
    return aus


def _clip():
    out = []
    for i in range(N):
        y, u, v = J.picture(W + 16, H, 3)
        data, _ = J.write_jpeg(J.subsample(*[np.ascontiguousarray(p[:, 2 * i:2 * i + W]) for p in (y, u, v)], "422"), "422", dri=3 if i & 1 else 0, dht=i != 2)
        out.append((data, J.decode(data)[1]))
    return out


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_jpeg_caps_give_the_stream_of_the_decoded_pictures(tmp_path, E):
    clip = _clip()
    jpeg_caps = "image/jpeg,width=%d,height=%d,framerate=30/1" % (W, H)
    got = _run(tmp_path, "jpeg", [d for d, _ in clip], jpeg_caps, N)
    # the same element on the planar 4:2:2 pictures the reference decodes, labelled the way a `jpegdec` in front would label them
    raw = [b"".join(np.ascontiguousarray(p).tobytes() for p in planes) for _, planes in clip]
    ref = _run(tmp_path, "raw", raw, "video/x-raw,format=Y42B,width=%d,height=%d,framerate=30/1,colorimetry=(string)1:4:0:0" % (W, H), N)
    assert got == ref
    (s,) = sps_of(got[0])
    assert s["colorimetry"] == (1, 2, 2, 6)  # full range, matrix 6
    # ... and the access units of the C ABI for the same pictures
    e = E.Encoder(W, H, fps=30, gop=4, fixed_qp=QP, colorimetry=(1, 2, 2, 6), slices=None, slice_deblock=None)
    abi = []
    for i, (d, _) in enumerate(clip):
        e.submit_jpeg(d, pts=i)
        abi.append(e.collect()[0])
    e.close()
    assert [bytes(a) for a in abi] == got
    # caps that carry a colorimetry override the default
    lim = _run(tmp_path, "bt601", [d for d, _ in clip[:2]], jpeg_caps + ",colorimetry=(string)bt601", 2)
    (s,) = sps_of(lim[0])
    assert s["colorimetry"] == (0, 6, 6, 6)


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_one_corrupt_buffer_is_dropped_and_the_rest_arrive(tmp_path):
    clip = [d for d, _ in _clip()]
    caps = "image/jpeg,width=%d,height=%d,framerate=30/1" % (W, H)
    bad = list(clip)
    bad[3] = clip[3][:len(clip[3]) // 2] + b"\xff\xd9"  # the data ends before the last MCU
    got = _run(tmp_path, "corrupt", bad, caps, N - 1)
    good = _run(tmp_path, "good", clip[:3] + clip[4:], caps, N - 1)
    assert got == good
