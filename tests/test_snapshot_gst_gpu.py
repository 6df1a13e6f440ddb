"""GPU: the element's snapshot-* properties (mi355enc_request_snapshot / _take_snapshot behind them) inside a GStreamer graph,
through ceracoder_amd/mi355_gst_probe: the file appears and is a JPEG of the reduced size, the bus carries `mi355-snapshot`, a reduction changed while
playing changes the next file's size, and the encoded stream is that of the run without the properties."""
import json
import os
import struct
import subprocess

import pytest

from tests import jpegref
from tests.test_boundary_cpu import PROBE, gst_env

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, N = 64, 48, 48  # 48 pictures at the probe's 60 pictures/s: 800 ms of stream time


def _run(tmp_path, name, props, args=()):
    out = tmp_path / (name + ".bin")
    desc = ("appsrc name=src ! video/x-raw,width=%d,height=%d,framerate=60/1,format=NV12 ! mi355h264enc qp=30 key-int-max=16 stats=true %s name=venc_bps ! "
            "appsink name=appsink sync=false" % (W, H, props))
    r = subprocess.run([PROBE, desc, "--appsrc", str(N), str(W), str(H), "--dump", str(out), "--stills"] + list(args), env=gst_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    data, aus, o = out.read_bytes(), [], 0
    while o < len(data):
        n, _, _ = struct.unpack_from("<III", data, o)
        aus.append(data[o + 12:o + 12 + n])
        o += 12 + n
    assert len(aus) == N
    lines = [json.loads(l) for l in r.stderr.splitlines() if l.startswith("{")]
    return aus, [l for l in lines if "still" in l], [l for l in lines if "snapshots" in l]


def test_element_writes_stills_and_leaves_the_stream_alone(tmp_path):
    loc = tmp_path / "preview.jpg"
    plain, none, counted = _run(tmp_path, "plain", "")
    assert not none and not counted and not loc.exists()
    for source in ("source", "decoded"):
        aus, stills, counted = _run(tmp_path, source, "snapshot-location=%s snapshot-interval=100 snapshot-reduce=4 snapshot-quality=60 snapshot-source=%s" % (loc, source),
                                    args=("--set", "20", "snapshot-reduce", "2"))
        assert aus == plain                                    # the encoded stream is that of the run without the properties
        assert stills and all(s["still"] == str(loc) and s["bytes"] > 600 for s in stills)
        assert counted and counted[0]["snapshots"] >= len(stills) >= 2
        sizes = [(s["width"], s["height"]) for s in stills]
        assert sizes[0] == (16, 12) and sizes[-1] == (32, 24), sizes   # armed every 100 ms = 6 pictures: the stills after picture 20 are reduced by 2
        assert [s["pts"] for s in stills] == sorted(s["pts"] for s in stills)
        hdr = jpegref.parse(loc.read_bytes())                  # the file that is there at the end: a whole baseline JPEG of the last still's size
        assert (hdr["width"], hdr["height"], hdr["components"], hdr["hs"], hdr["vs"]) == (32, 24, 3, 2, 2)
        assert loc.read_bytes()[-2:] == b"\xff\xd9" and not (tmp_path / "preview.jpg.tmp").exists()
        loc.unlink()


def test_a_location_that_cannot_be_written_is_a_warning_not_an_error(tmp_path):
    aus, stills, counted = _run(tmp_path, "nowhere", "snapshot-location=%s snapshot-interval=100" % (tmp_path / "no_such_dir" / "x.jpg"))
    assert len(aus) == N and not stills and not counted
