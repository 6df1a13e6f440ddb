"""GPU: the image layer inside a GStreamer graph -- `mi355h264enc` with image-location (a PAM file), image-offset-x / -y and image-alpha, the drop-in for a
`gdkpixbufoverlay` in front of the encoder, against the Python path with the same layer; driven like tests/test_overlay_gst_gpu.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import imageref as R
from tests.spsref import sps_of
from tests.test_boundary_cpu import HARNESS, gst_env
from tests.test_scale_gpu import clip

pytestmark = pytest.mark.gpu

W, H, QP, N, GOP = 208, 120, 28, 5, 4
X, Y, ALPHA = 21, -6, 0.3


def _run(tmp_path, name, blocks, props):
    src, pf, out = tmp_path / (name + ".src"), tmp_path / name, tmp_path / (name + ".bin")
    src.write_bytes(b"".join(blocks))
    pf.write_text("filesrc location=%s blocksize=%d ! video/x-raw,format=NV12,width=%d,height=%d,framerate=30/1 ! mi355h264enc qp=%d key-int-max=%d %s name=venc_bps"
                  " ! appsink name=appsink sync=false\n" % (src, len(blocks[0]), W, H, QP, GOP, props))
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data, aus, o = out.read_bytes(), [], 0
    while o < len(data):  # records {u32 length, u64 pts_ns, bytes}
        n, _ = struct.unpack_from("<IQ", data, o)
        aus.append(data[o + 12:o + 12 + n])
        o += 12 + n
    assert len(aus) == len(blocks)
    return aus, r.stderr


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_element_with_an_image_gives_the_python_paths_stream(tmp_path, E):
    pics = clip(W, H, N)
    blocks = [y.tobytes() + uv.tobytes() for y, uv in pics]
    img = R.random_image(np.random.default_rng(12), 64, 40)
    pam = tmp_path / "logo.pam"
    pam.write_bytes(R.pam(img))
    got, _ = _run(tmp_path, "image", blocks, "image-location=%s image-offset-x=%d image-offset-y=%d image-alpha=%s" % (pam, X, Y, ALPHA))
    plain, _ = _run(tmp_path, "plain", blocks, "")
    assert got != plain and got[0] != plain[0]
    (s,) = sps_of(got[0])
    opacity = 77  # rint(256 * 0.3)

    def abi(with_layer):
        e = E.Encoder(W, H, fps=30, gop=GOP, fixed_qp=QP, colorimetry=s["colorimetry"], slices=None, slice_deblock=None)
        if with_layer:
            e.set_image(0, img, X, Y, opacity, E.FMT_RGBX)
        out = [e.encode(y, uv, pts=i)[0] for i, (y, uv) in enumerate(pics)]
        e.close()
        return out
    assert plain == abi(False)
    assert got == abi(True)
    # a file the reader refuses, and one that is not there: a warning each, and the stream of a plain encoder; "" switches the layer off
    bad = tmp_path / "bad.pam"
    bad.write_bytes(R.pam(img).replace(b"MAXVAL 255", b"MAXVAL 65535"))
    for name, loc in (("bad", bad), ("missing", tmp_path / "none.pam")):
        aus, _ = _run(tmp_path, name, blocks, "image-location=%s" % loc)
        assert aus == plain, name
