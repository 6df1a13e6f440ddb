"""GPU: frame-rate conversion inside the element: the buffers that leave lie on the output rate's grid, the source caps carry that
rate, repeats leave as buffers of their own, and the stream decodes.  Driven by oracle/_ref/ref_harness like the element's other graph tests."""
import json
import os
import subprocess

import pytest

from tests.test_boundary_cpu import HARNESS, gst_env
from tests.test_gst_gpu import read_records

pytestmark = pytest.mark.gpu
NS = 10 ** 9


def run(tmp_path, text):
    pf, out = tmp_path / "pipe", tmp_path / "out.bin"
    pf.write_text(text)
    r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.splitlines()[-1]), read_records(str(out))


def decodes(oracle, recs, size):
    dec = oracle.Decoder()
    for _, au in recs:
        y, _ = dec.decode(au)
    assert dec.size == size and 20 < float(y[:size[1], :size[0]].mean()) < 235


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_blend_50_to_30_leaves_on_the_30_hz_grid(tmp_path, oracle):
    """20 pictures at 50/1 (the last at 380 ms) make the ticks 0 .. 11 due.  The capsfilter behind the element only links when the source caps say 30/1."""
    summary, recs = run(tmp_path, "videotestsrc num-buffers=20 pattern=ball ! video/x-raw,width=320,height=180,framerate=50/1,format=NV12 ! "
                                  "mi355h264enc rate-conversion=blend output-framerate=30/1 pipeline-depth=2 key-int-max=30 qp=26 name=venc_bps ! "
                                  "video/x-h264,framerate=30/1 ! appsink name=appsink sync=false\n")
    assert summary["samples"] == 12 and summary["pts_backwards"] == 0 and summary["pts_repeated"] == 0
    t0 = recs[0][0]
    assert [p - t0 for p, _ in recs] == [k * NS // 30 for k in range(12)]
    decodes(oracle, recs, (320, 180))


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_hold_30_to_60_pushes_the_repeats_in_order(tmp_path, oracle):
    """10 pictures at 30/1: every one but the first is preceded by a repeat of the one before it -- 19 buffers, each with its own tick's PTS, in order"""
    summary, recs = run(tmp_path, "videotestsrc num-buffers=10 pattern=ball ! video/x-raw,width=320,height=180,framerate=30/1,format=I420 ! "
                                  "mi355h264enc rate-conversion=hold output-framerate=60/1 pipeline-depth=2 key-int-max=30 qp=26 name=venc_bps ! "
                                  "video/x-h264,framerate=60/1 ! appsink name=appsink sync=false\n")
    assert summary["samples"] == 19 and summary["pts_backwards"] == 0 and summary["pts_repeated"] == 0
    t0 = recs[0][0]
    assert [p - t0 for p, _ in recs] == [k * NS // 60 for k in range(19)]
    # (a repeat costs next to nothing and the picture behind it a lot: the scene-cut rule may well force an IDR picture among them)
    assert recs[0][1][:5] == b"\x00\x00\x00\x01\x67" and all(au[:5] in (b"\x00\x00\x00\x01\x67", b"\x00\x00\x00\x01\x41") for _, au in recs[1:])
    decodes(oracle, recs, (320, 180))
