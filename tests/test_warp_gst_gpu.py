"""GPU: lens, roll and keystone correction inside a GStreamer graph -- `mi355h264enc`'s lens-k1, lens-k2, lens-zoom, roll, keystone-h, keystone-v and warp-filter
(DESIGN.md section 27), in the manner of tests/test_denoise_gst_gpu.py, driven through the project's own probe program: with values that are exact in Q16 the
element's stream is the C ABI's for the same integers; a roll written while playing changes the stream from the next picture on without a new IDR picture."""
import os

import pytest

from ceracoder_amd import synth
from tests.spsref import sps_of
from tests.test_boundary_cpu import PROBE
from tests.test_orient_gst_gpu import RAW, _abi, _raw, _run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(PROBE), reason="ceracoder_amd/mi355_gst_probe not built (no GStreamer)")]

W, H, N = 160, 96, 8
P41, SPS = b"\x00\x00\x00\x01\x41", b"\x00\x00\x00\x01\x67"


def clip():
    import numpy as np
    return [(np.ascontiguousarray(y[:H, :W]), np.ascontiguousarray(uv[:H // 2, :W])) for y, uv in synth.s2_frames(W, H, N)]


def test_lens_and_keystone_properties_give_the_abi_stream_of_the_same_integers(tmp_path, E):
    pics = clip()
    got = _run(tmp_path, "lens", _raw(pics), RAW % (W, H), "lens-k1=-0.203125 lens-k2=0.03125 keystone-h=0.125", gop=60)
    col = sps_of(got[0][0])[0]["colorimetry"]

    def feed(e, i):
        if i == 0:
            e.set_warp(dict(kind=E.WARP_BICUBIC, fill=(16, 128, 128)), k1=-13312, k2=2048, kh=8192)  # (border-color's default is black)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in got] == _abi(E, W, H, col, feed, N, gop=60)
    plain = _abi(E, W, H, col, lambda e, i: e.submit(*pics[i], pts=i), N, gop=60)
    assert [g[0] for g in got] != plain
    neutral = _run(tmp_path, "neutral", _raw(pics), RAW % (W, H), "lens-zoom=1 roll=0 warp-filter=bilinear", gop=60)  # all neutral: off
    assert [g[0] for g in neutral] == plain
    bilinear = _run(tmp_path, "bil", _raw(pics), RAW % (W, H), "keystone-v=-0.125 warp-filter=bilinear border-color=4217544", gop=60)

    def feed_b(e, i):
        if i == 0:
            e.set_warp(dict(kind=E.WARP_BILINEAR, fill=(0x40, 0x5A, 0xC8)), kv=-8192)
        e.submit(*pics[i], pts=i)
    assert [g[0] for g in bilinear] == _abi(E, W, H, col, feed_b, N, gop=60)


def test_a_roll_written_while_playing_takes_the_next_picture_without_a_new_idr(tmp_path, E, oracle):
    pics = clip()
    props = "scenecut=false"  # (the rolled picture is a new picture to the scene-cut rule, which may answer with an IDR picture of its own)
    still = _run(tmp_path, "still", _raw(pics), RAW % (W, H), props, gop=60)
    got = _run(tmp_path, "roll", _raw(pics), RAW % (W, H), props, args=("--set", "4", "roll", "3.5"), gop=60)
    assert [g[0] for g in got[:4]] == [g[0] for g in still[:4]]
    assert all(g[0] != s[0] for g, s in zip(got[4:], still[4:]))
    assert got[0][0][:5] == SPS and all(g[0][:5] == P41 for g in got[1:])  # one IDR picture, one set of parameter sets
    assert all((w, h) == (W, H) for _, w, h in got)
    dec = oracle.Decoder()  # (the roll's own bytes are not pinned: its cos / sin come from libm)
    for au, _, _ in got:
        y, _ = dec.decode(au)
    assert dec.size == (W, H) and 20 < float(y[:H, :W].mean()) < 235
