"""CPU: the input geometry on the host -- the tables mi355enc_geometry_table builds against tests/geomref.py and, in the degenerate
case, against mi355enc_scale_table; mi355enc_fit_rect against its formula; the validity rule; the sample aspect ratio and the SPS it gives.  No device needed."""
import numpy as np
import pytest

from tests import geomref as G

KINDS = [G.LUMA, G.CHROMA_V, G.CHROMA_H, G.CHROMA_V422]
# (crop, dst) per ratio s = crop / dst: 1/8, 2/5, 1/2, 1, 5/4, 8
RATIOS = [(16, 128), (40, 100), (64, 128), (96, 96), (120, 96), (256, 32)]


@pytest.mark.parametrize("n_in,n_out", [(3840, 1920), (1918, 642), (1080, 480), (64, 64), (256, 32), (1366, 1024)])
@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_tables_equal_the_restatement_and_the_scaler(E, n_in, n_out, kind):
    first, coef = E.geometry_table(0, n_in, n_out, kind)
    rf, rc = G.padded(G.table(0, n_in, n_out, kind))
    assert first.shape == rf.shape and np.array_equal(first, rf)
    assert coef.shape == rc.shape and np.array_equal(coef, rc), np.argwhere(coef != rc)[:4]
    sf, sc = E.scale_table(n_in, n_out, kind)
    assert np.array_equal(first, sf) and coef.shape == sc.shape and np.array_equal(coef, sc)


@pytest.mark.parametrize("crop,dst", RATIOS, ids=lambda v: str(v))
@pytest.mark.parametrize("off", [0, 2, "far"])
@pytest.mark.parametrize("kind", KINDS)
def test_tables_equal_the_restatement(E, crop, dst, off, kind):
    if off == "far":  # a crop that touches the far edge of a 400-sample picture
        off = 400 - crop
    first, coef = E.geometry_table(off, crop, dst, kind)
    rf, rc = G.padded(G.table(off, crop, dst, kind))
    assert first.shape == rf.shape and np.array_equal(first, rf), np.argwhere(first != rf)[:4]
    assert coef.shape == rc.shape and np.array_equal(coef, rc), np.argwhere(coef != rc)[:4]
    assert (coef.astype(np.int64).sum(axis=1) == 1 << 14).all()
    if crop <= dst and kind != G.CHROMA_V422:  # upscaling: the unstretched kernel
        assert coef.shape[1] <= 4
    assert np.abs(coef.astype(np.int64)).sum(axis=1).max() <= 1.25 * (1 << 14) or crop > dst


@pytest.mark.parametrize("src,target", [((1080, 1920), (1920, 1080)), ((640, 480), (1280, 720)), ((1920, 1080), (1920, 1080)), ((2, 2), (16, 16)),
                                        ((1920, 1080), (1280, 1024)), ((1, 4000), (64, 64))])
def test_fit_rect(E, src, target):
    got = E.fit_rect(src[0], src[1], target[0], target[1])
    assert got == G.fit_rect(src[0], src[1], target[0], target[1])
    dx, dy, dw, dh = got
    assert not any(v % 2 for v in got) and dx >= 0 and dy >= 0 and dx + dw <= target[0] and dy + dh <= target[1]
    assert dw == target[0] or dh == target[1]


def test_fit_rect_known_answers(E):
    assert E.fit_rect(1080, 1920, 1920, 1080) == (656, 0, 608, 1080)
    assert E.fit_rect(640, 480, 1280, 720) == (160, 0, 960, 720)
    assert E.fit_rect(1920, 1080, 1920, 1080) == (0, 0, 1920, 1080)
    assert E.fit_rect(2, 2, 16, 16) == (0, 0, 16, 16)


GOOD = dict(in_size=(160, 96), crop=(18, 10, 120, 70), dst=(22, 6, 100, 36))
BAD = [
    dict(in_size=(161, 96)), dict(crop=(17, 10, 120, 70)), dict(crop=(18, 10, 120, 71)), dict(dst=(22, 6, 100, 35)), dict(dst=(21, 6, 100, 36)),  # odd
    dict(crop=(42, 10, 120, 70)), dict(crop=(18, 28, 120, 70)), dict(dst=(46, 6, 100, 36)), dict(dst=(22, 14, 100, 36)),  # outside the picture
    dict(crop=(-2, 10, 120, 70)), dict(dst=(22, -2, 100, 36)), dict(crop=(18, 10, 0, 70)), dict(dst=(22, 6, 100, 0)),
    dict(crop=(18, 10, 120, 70), dst=(22, 6, 14, 36)), dict(crop=(18, 10, 120, 70), dst=(22, 6, 100, 8)),  # crop > 8 dst
    dict(crop=(18, 10, 12, 70)), dict(crop=(18, 10, 120, 4)),  # dst > 8 crop
    dict(in_size=(8194, 96)), dict(border=(256, 128, 128)),
]


def test_the_validity_rule_accepts_the_good_geometry(E):
    assert E.geometry_valid(E.geometry(**GOOD), 144, 48)
    assert G.valid(160, 96, GOOD["crop"], GOOD["dst"], 144, 48)
    assert E.geometry_valid(E.geometry((128, 128), crop=(0, 0, 128, 128), dst=(0, 0, 16, 16)), 16, 16)  # a ratio of exactly 8, both ways
    assert E.geometry_valid(E.geometry((16, 16), dst=(0, 0, 128, 128)), 128, 128)


@pytest.mark.parametrize("change", BAD, ids=lambda c: str(c))
def test_the_validity_rule_refuses(E, change):
    kw = dict(GOOD)
    kw.update(change)
    assert not E.geometry_valid(E.geometry(**kw), 144, 48)
    if "border" not in change:
        assert not G.valid(kw["in_size"][0], kw["in_size"][1], kw["crop"], kw["dst"], 144, 48)


def test_table_refuses_what_the_rule_refuses(E):
    for off, crop, dst in [(1, 16, 16), (0, 15, 16), (0, 16, 15), (-2, 16, 16), (0, 130, 16), (0, 16, 130), (0, 0, 16)]:
        with pytest.raises(E.EncoderError):
            E.geometry_table(off, crop, dst, G.LUMA)
    for n_in, n_out in [(16, 32), (640, 1280)]:  # the scaler's own table keeps its contract: no upscaling
        with pytest.raises(E.EncoderError):
            E.scale_table(n_in, n_out, G.LUMA)


SAR_CASES = [((0, 0, 160, 96), (0, 0, 160, 96)), ((18, 10, 120, 70), (22, 6, 100, 36)), ((0, 0, 1080, 1920), (656, 0, 608, 1080)),
             ((0, 0, 640, 480), (160, 0, 960, 720)), ((0, 0, 3840, 2160), (0, 0, 1920, 1080)), ((0, 0, 1440, 1080), (0, 0, 1920, 1080))]


@pytest.mark.parametrize("crop,dst", SAR_CASES, ids=lambda v: str(v))
def test_sar_exact_by_default_absent_with_keep_sar_exchanged_when_transposed(E, crop, dst):
    size = (crop[0] + crop[2], crop[1] + crop[3])
    g = E.geometry(size, crop=crop, dst=dst)
    want = G.sar(crop, dst)
    assert E.geometry_sar(g) == want
    assert E.geometry_sar(g, transposed=True) == G.sar(crop, dst, transposed=True) == (None if want is None else (want[1], want[0]))
    k = E.geometry(size, crop=crop, dst=dst, keep_sar=True)
    assert E.geometry_sar(k) is None and E.geometry_sar(k, transposed=True) is None and G.sar(crop, dst, keep_sar=True) is None
    # the SPS: the host writer's with that ratio; without one, byte for byte the headers of an unscaled stream
    plain = E.host_write_headers(1920, 1080, 30)
    assert E.host_write_headers(1920, 1080, 30, sar=E.geometry_sar(k)) == plain
    if want is not None:
        from tests import spsref
        hdr = E.host_write_headers(1920, 1080, 30, sar=E.geometry_sar(g))
        assert hdr != plain and spsref.sps_of(hdr)[0]["sar"] == want


def test_sar_of_the_pillarbox_is_what_fit_rect_rounded(E):
    """1080 x 1920 into 608 x 1080: (1080 * 1080) : (1920 * 608) = 1215 : 1216 -- the ratio KEEP_SAR exists to keep out of the VUI"""
    g = E.geometry((1080, 1920), dst=E.fit_rect(1080, 1920, 1920, 1080))
    assert E.geometry_sar(g) == (1215, 1216)


def test_geometry_entry_points_are_exported(E):
    L = E.load()
    for name in ("mi355enc_set_input_geometry", "mi355enc_get_input_geometry", "mi355enc_set_crop", "mi355enc_geometry_table", "mi355enc_fit_rect",
                 "mi355enc_stage_geometry", "mi355enc_geometry_check", "mi355enc_geometry_sar"):
        assert name in E.EXPORTS and getattr(L, name)
