"""GPU: electronic image stabilisation inside a GStreamer graph -- `mi355h264enc`'s stabilize, stabilize-range and stabilize-leak, in the
manner of tests/test_geometry_gst_gpu.py, driven through the project's own probe program: with the properties set the element's stream is the mirror's for
the same geometry and setting, at the reduced size; at their defaults nothing changes."""
import os

import pytest

from tests import stabref as S
from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import RAW, _abi, _raw, _run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, N = 160, 96, 8


def test_stabilize_reduces_the_size_and_is_the_mirrors_stream(tmp_path, E):
    pics = S.clip(W, H)[:N]
    recs = S.run([p[0] for p in pics], (8, 16, 16, 16), (16, 16, W - 32, H - 32), W, H)
    assert all((r["mx"], r["my"]) == m and r["votes_x"] >= 3 and r["votes_y"] >= 3 for r, m in zip(recs[1:], S.SCRIPT[1:])) and len({r["ox"] for r in recs}) >= 4
    got = _run(tmp_path, "stab", _raw(pics), RAW % (W, H), "stabilize=17 stabilize-range=8", gop=60)  # (17 counts as 16)
    assert [(w, h) for _, w, h in got] == [(W - 32, H - 32)] * N  # the input less twice the margin
    (s,) = sps_of(got[0][0])
    g = E.geometry((W, H), crop=(16, 16, W - 32, H - 32), target=(W - 32, H - 32))
    seen = []

    def feed(e, i):
        e.submit(*pics[i], pts=i)
        if i:
            seen.append(e.last_stabilize()[1])  # (of the picture before: collected by then)
    abi = _abi(E, W - 32, H - 32, s["colorimetry"], feed, N, gop=60, geometry=g, stabilize=dict(range=8, leak=16, margin=16))
    assert seen == recs[:N - 1]
    assert [a for a, _, _ in got] == abi
    plain = _run(tmp_path, "crop", _raw(pics), RAW % (W, H), "crop-left=16 crop-right=16 crop-top=16 crop-bottom=16", gop=60)
    assert plain[0][0] == got[0][0] and plain[1][0] != got[1][0]  # the priming picture does not move; the next one does


def test_defaults_change_nothing(tmp_path):
    pics = S.clip(W, H)[:4]
    for props, defaults in (("", "stabilize=0 stabilize-range=16 stabilize-leak=16"), ("crop-left=16 crop-top=8", "stabilize-range=4 stabilize-leak=200")):  # (no margin: off)
        assert _run(tmp_path, "with", _raw(pics), RAW % (W, H), props + " " + defaults) == _run(tmp_path, "without", _raw(pics), RAW % (W, H), props)
