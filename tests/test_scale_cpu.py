"""CPU: the downscaling tables the library builds on the host (mi355enc_scale_table) against tests/scaleref.py, their invariants, and
hand-worked cases of the rule.  No device needed."""
import numpy as np
import pytest

from tests import scaleref as R

KINDS = [R.LUMA, R.CHROMA_V, R.CHROMA_H, R.CHROMA_V422]
PAIRS = [(3840, 1920), (3840, 1280), (3840, 640), (2160, 1080), (2160, 720), (2160, 360), (1920, 1280), (1920, 854), (1080, 720),
         (1080, 480), (2560, 1920), (1440, 1080), (1918, 642), (1078, 362), (1280, 960), (1920, 240), (16, 16), (1920, 1920), (64, 10),
         (7680, 960), (1366, 1024)]


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_host_tables_equal_the_restatement(E, n_in, n_out, kind):
    first, coef = E.scale_table(n_in, n_out, kind)
    rf, rc = R.padded(R.table(n_in, n_out, kind))
    assert first.shape == rf.shape and np.array_equal(first, rf)
    assert coef.shape == rc.shape and np.array_equal(coef, rc), np.argwhere(coef != rc)[:4]


@pytest.mark.parametrize("n_in,n_out", PAIRS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_phase_sums_to_2_14(E, n_in, n_out, kind):
    _, coef = E.scale_table(n_in, n_out, kind)
    assert (coef.astype(np.int64).sum(axis=1) == 1 << 14).all()


@pytest.mark.parametrize("n", [16, 360, 1080, 1920])
def test_unit_stretch_is_the_identity(E, n):
    for kind in (R.LUMA, R.CHROMA_V):
        first, coef = E.scale_table(n, n, kind)
        m = n if kind == R.LUMA else n // 2
        assert np.array_equal(first, np.arange(m) - 1)
        assert (coef[:, 1] == 1 << 14).all() and (coef[:, 0] == 0).all() and (coef[:, 2:] == 0).all()


def _tables(in_w, in_h, out_w, out_h):
    return R.table(in_w, out_w, R.LUMA), R.table(in_h, out_h, R.LUMA)


@pytest.mark.parametrize("value", [0, 17, 128, 255])
def test_constant_plane_stays_constant(E, value):
    for in_w, in_h, out_w, out_h in [(3840, 2160, 1280, 720), (1918, 1078, 642, 362), (64, 64, 8, 8)]:
        th = [(f, q) for f, q in zip(*E.scale_table(in_w, out_w, R.LUMA))]
        tv = [(f, q) for f, q in zip(*E.scale_table(in_h, out_h, R.LUMA))]
        out = R.scale_plane(np.full((in_h, in_w), value, np.uint8), th, tv)
        assert (out == value).all()


def test_halving_a_linear_ramp_gives_the_midpoints(E):
    """2:1 of f(x) = x: output i sits at 2i + 0.5; Catmull-Rom reproduces a linear ramp exactly, so away from the clamped edges the
    result is that midpoint up to the integer path's rounding."""
    w, h = 256, 32
    ramp = np.tile(np.arange(w, dtype=np.uint8)[None, :], (h, 1))
    th = [(f, q) for f, q in zip(*E.scale_table(w, w // 2, R.LUMA))]
    tv = [(f, q) for f, q in zip(*E.scale_table(h, h, R.LUMA))]
    out = R.scale_plane(ramp, th, tv).astype(np.int64)
    mid = 2 * np.arange(w // 2) + 0.5
    inner = slice(2, w // 2 - 2)
    assert (np.abs(out[:, inner] - mid[inner]) <= 1).all()


@pytest.mark.parametrize("n_in,n_out", [(1280, 1920), (1922, 240), (1919, 640), (1920, 641), (0, 0), (16, 18)])
def test_host_table_refuses_upscaling_large_ratios_and_odd_sizes(E, n_in, n_out):
    for kind in KINDS:
        with pytest.raises(E.EncoderError):
            E.scale_table(n_in, n_out, kind)


def test_ratio_of_exactly_8_is_accepted(E):
    """s = 8: 32 taps per luma sample (|j - c| < 16); 4:2:2 chroma rows stretch by 16: 64 taps"""
    assert E.scale_table(3840, 480, R.LUMA)[1].shape == (480, 32)
    assert E.scale_table(2160, 270, R.CHROMA_V422)[1].shape == (135, 64)


def test_scale_entry_points_are_exported(E):
    for name in ("mi355enc_set_input_size", "mi355enc_stage_scale", "mi355enc_scale_table"):
        assert name in E.EXPORTS and hasattr(E.load(), name)


@pytest.mark.parametrize("line,want", [("mi355h264enc", (0, 0)), ("mi355h264enc width=1280 height=720", (1280, 720)),
                                       ("mi355h264enc speed-preset=2 width=854 height=480", (854, 480))])
def test_element_width_and_height_properties_read_back(line, want):
    """mpph265enc-style `width` / `height` (0, the default: the input's size), read back through GObject; no device involved."""
    import json
    import subprocess
    from tests.test_boundary_cpu import PROBE, gst_env
    r = subprocess.run([PROBE, "videotestsrc ! %s name=venc_kbps ! appsink name=appsink" % line, "--props"], env=gst_env(), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.splitlines()[-1])
    assert (got["width"], got["height"]) == want


def test_camlink_720p_pipeline_scales_in_the_encoder():
    """pipeline/mi355x/x264_superfast_camlink_720p: the jetson line's `nvvidconv ... width=1280,height=720 ! nvvidconv ! x264enc` is the
    encoder alone, scaling on the GPU."""
    import os
    from tests.test_boundary_cpu import ROOT
    text = open(os.path.join(ROOT, "pipeline", "mi355x", "x264_superfast_camlink_720p")).read()
    line = [l for l in text.splitlines() if l.startswith("mi355h264enc")][0]
    assert line.rstrip(" !") == "mi355h264enc width=1280 height=720 speed-preset=2 key-int-max=60 name=venc_kbps"
    assert "nvvidconv" not in text and "videoscale" not in text
