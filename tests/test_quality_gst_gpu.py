"""GPU: the element's quality-stats property (mi355enc_set_quality_metrics behind it) inside a GStreamer graph, driven like tests/test_gst_gpu.py."""
import json
import math
import os
import subprocess

import pytest

from tests.test_boundary_cpu import HARNESS, gst_env

pytestmark = pytest.mark.gpu


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_quality_stats_prints_the_streams_psnr_and_ssim(tmp_path):
    """quality-stats=true stats=true: the summary gains one line with the stream's PSNR of Y, Cb, Cr and mean SSIM, finite and in range;
    without the property the line is absent."""
    lines = {}
    for on in (True, False):
        pf = tmp_path / ("pipe%d" % on)
        pf.write_text("videotestsrc num-buffers=12 pattern=ball ! video/x-raw,width=320,height=192,framerate=30/1,format=NV12 ! "
                      "mi355h264enc qp=30 stats=true %sname=venc_bps ! appsink name=appsink sync=false\n" % ("quality-stats=true " if on else ""))
        r = subprocess.run([HARNESS, str(pf), str(tmp_path / "out.bin")], env=gst_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[on] = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{\"element\"")]
    assert len(lines[False]) == 1 and "quality" not in lines[False][0]
    assert len(lines[True]) == 2 and lines[True][0]["frames"] == 12
    q = lines[True][1]["quality"]
    assert q["pictures"] == 12
    for k in ("psnr_y", "psnr_cb", "psnr_cr"):
        assert math.isfinite(q[k]) and 20.0 < q[k] <= 100.0, q
    assert math.isfinite(q["ssim"]) and 0.5 < q["ssim"] <= 1.0, q
