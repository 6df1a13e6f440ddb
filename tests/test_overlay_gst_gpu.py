"""GPU: the text overlay inside a GStreamer graph -- `mi355textoverlay` (the drop-in for the reference's `textoverlay ... name=overlay`) handing its
text to `mi355h264enc` by event, against the encoder's own overlay-text property; driven like tests/test_quality_gst_gpu.py."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import overlayref as R
from tests.test_boundary_cpu import HARNESS, gst_env

pytestmark = pytest.mark.gpu

W, H, QP, N = 320, 240, 24, 5
TEXT = "b: 2048/ 1900 rtt:  40"
SRC = "videotestsrc num-buffers=%d ! video/x-raw,width=%d,height=%d,framerate=30/1,format=NV12 ! " % (N, W, H)
SINK = " ! appsink name=appsink sync=false\n"


def _run(tmp_path, name, middle):
    pf, out = tmp_path / name, tmp_path / (name + ".bin")
    pf.write_text(SRC + middle + SINK)
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data, aus, o = out.read_bytes(), [], 0
    while o < len(data):  # records {u32 length, u64 pts_ns, bytes}
        n, _ = struct.unpack_from("<IQ", data, o)
        aus.append(data[o + 12:o + 12 + n])
        o += 12 + n
    assert len(aus) == N
    return aus


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_textoverlay_element_and_property_draw_the_same_text(tmp_path, oracle):
    by_event = _run(tmp_path, "event", "mi355textoverlay text=\"%s\" valignment=top halignment=right font-desc=\"Monospace, 5\" name=overlay ! queue ! "
                                       "mi355h264enc qp=%d key-int-max=60 name=venc_bps" % (TEXT, QP))
    by_prop = _run(tmp_path, "prop", "mi355h264enc qp=%d key-int-max=60 overlay-text=\"%s\" name=venc_bps" % (QP, TEXT))
    plain = _run(tmp_path, "plain", "mi355h264enc qp=%d key-int-max=60 name=venc_bps" % QP)
    assert by_event == by_prop
    assert by_event != plain and by_event[0] != plain[0]
    # The first, IDR picture through the independent decoder: text samples against outline samples.  In the source they are 235 and 16, 219 apart.
    # QP 24 and the margin come from the CPU oracle's reconstruction of pictures with this text drawn in by overlayref at this size (a synthetic
    # clip, a flat white picture, noise): every text sample came out >= 223 and every outline sample <= 29 there, 194 apart in the worst case (QP 30:
    # 171, QP 36: 117).  Asked for here: the darkest text sample at least 128 above the brightest outline sample -- more than half the source's contrast.
    dy, _ = oracle.Decoder().decode(by_event[0])
    T, O, _ = R.masks(TEXT, W, H)
    t, o = dy[:H, :W][T].astype(int), dy[:H, :W][O].astype(int)
    print("text min %d mean %.1f, outline max %d mean %.1f" % (t.min(), t.mean(), o.max(), o.mean()))
    assert t.min() - o.max() >= 128, (t.min(), o.max())
    py, _ = oracle.Decoder().decode(plain[0])
    assert not np.array_equal(py, dy)
