"""Conditions on the inputs of tests/test_size_range_gpu.py, asserted on the oracle's records alone (tests/sizerange.py): the strips at the ends of the accepted
size range carry, in every P picture, the content the kernels' width- and height-dependent structures are about -- intra macroblocks in the last column / row
and beyond index 480 (the last word of the intra rows' bit sets), coded and refined inter macroblocks beyond index 256, skipped macroblocks -- and the band
deblocker's cut finds bands with and without a free column on them."""
import numpy as np
import pytest

from tests import cutref
from tests import sizerange as S


def _along(records, w, h):
    """the records as (across, along): the strip's long axis last"""
    mbw, mbh = S.mb_size(w, h)
    g = records.reshape(mbh, mbw)
    return g if S.is_wide(w, h) else g.T


def test_the_tables_are_what_their_comments_say():
    assert all(w % 2 == 0 and h % 2 == 0 and 16 <= w <= 8192 and 16 <= h <= 8192 for w, h in S.STRIPS + S.THRESHOLDS + S.INPUT_SHAPES)
    assert [S.mb_size(w, h)[0] for w, h in S.WIDE] == [512, 512, 512, 257, 511, 512] and [S.mb_size(w, h)[1] for w, h in S.TALL] == [512, 512, 512, 257, 512]
    assert S.mb_size(8192, 144) == (512, 9) and 512 * 9 == 4608 > 4096                      # three bands, the last of one row; the <8> scan
    assert [a * b for a, b in (S.mb_size(w, h) for w, h in S.THRESHOLDS)] == [4096, 4160, 8192, 8256, 32768, 32896]
    assert -(-32896 // 1024) == 33                                                           # qp_chain_kernel's macroblocks per thread at the largest
    cells = [S.grid_size(a, b) for a, b in S.grid_cells("full")]
    assert len(cells) == 81 and cells[0] == (16, 16) and cells[-1] == (142, 142) and all(S.mb_size(*c) == ab for c, ab in zip(cells, S.grid_cells("full")))
    frame = S.grid_cells("frame")
    assert len(frame) == 32 + 7 and set(frame) <= set(S.grid_cells("full")) and all((a, a) in frame for a in S.GRID)


@pytest.mark.parametrize("w,h", S.STRIPS)
def test_strip_clip_reaches_the_far_end(oracle, w, h):
    """Every P picture of strip_clip at QP 30 (IDR + three P pictures; the decoder's output equalled the reconstruction: sizerange.oracle_stream)."""
    st = S.fixed_qp_stream(oracle, w, h)
    assert st[0][1] and not any(s[1] for s in st[1:])
    n_along = max(S.mb_size(w, h))
    for i, (_, _, _, _, rec) in enumerate(st[1:], 1):
        g = _along(rec, w, h)
        idx = np.broadcast_to(np.arange(g.shape[1]), g.shape)
        intra = g["mb_type"] != 1
        coded = ~intra & (g["nzmask"] != 0)
        quarter = ~intra & ((g["mvx"] % 4 != 0) | (g["mvy"] % 4 != 0))
        assert intra[:, -1].any(), (i, "no intra macroblock at the far end")
        if n_along >= 488:
            assert (intra & (idx >= 480)).sum() >= 8, (i, int((intra & (idx >= 480)).sum()))
        # (4112: mbw 257 -- index 256 is the only one that far, and it lies in the flat patch that makes it intra)
        if n_along > 256 + 13:
            assert (coded & (idx >= 256)).any() and (quarter & (idx >= 256)).any(), i
        assert (~intra & (g["nzmask"] == 0)).any(), (i, "no skipped macroblock")


@pytest.mark.parametrize("w,h", S.WIDE)
def test_strip_streams_have_bands_with_and_without_a_cut(oracle, w, h):
    """The P pictures of the strip's Baseline stream (the QPs of extremes.STREAM_QPS), through tests/cutref.py: some band is cut inside the row, and some band
    is not (no free column in the window, or nothing to filter)."""
    mbw, mbh = S.mb_size(w, h)
    assert mbw >= cutref.DB_CUT_MIN_MBW
    cuts = np.concatenate([cutref.expected_cuts(rec, mbw, mbh)[:, 0] for _, key, _, _, rec in S.strip_stream(oracle, "baseline", w, h) if not key])
    assert ((cuts > 0) & (cuts < mbw)).any() and ((cuts == 0) | (cuts == mbw)).any(), cuts.tolist()


def test_tall_strips_are_past_the_room_for_device_side_waits():
    """the strips fall on both sides of the launch size up to which kernels may wait for each other on the device; every size another GPU test runs with three
    pictures in flight stays on the near side"""
    assert all(S.wait_wgs(*S.mb_size(w, h)) <= S.WAIT_WGS_MAX for w, h in S.WIDE) and all(S.wait_wgs(*S.mb_size(w, h)) > S.WAIT_WGS_MAX for w, h in S.TALL)
    assert [S.wait_wgs(*S.mb_size(w, h)) for w, h in ((16, 8192), (32, 4112), (144, 8192))] == [768, 387, 256]
    assert all(S.wait_wgs(*S.mb_size(w, h)) <= S.WAIT_WGS_MAX for w, h in ((1920, 1080), (3840, 2160), (4096, 2304), (960, 256), (1280, 720)))


def test_tall_strips_are_below_the_cut():
    assert all(S.mb_size(w, h)[0] < cutref.DB_CUT_MIN_MBW for w, h in S.TALL)


def test_remainder_sweep_has_every_kind_of_macroblock(oracle):
    """Over the P pictures of the 81 geometries: intra, coded inter and skipped macroblocks (measured: 507 / 4627 / 941 of 6075)."""
    n = intra = coded = skip = 0
    for mbw, mbh in S.grid_cells("full"):
        for _, key, _, _, rec in S.grid_stream(oracle, "baseline-depth0", mbw, mbh):
            if not key:
                n += rec.size
                intra += int((rec["mb_type"] != 1).sum())
                coded += int(((rec["mb_type"] == 1) & (rec["nzmask"] != 0)).sum())
                skip += int(((rec["mb_type"] == 1) & (rec["nzmask"] == 0)).sum())
    assert n == 3 * sum(a * b for a, b in S.grid_cells("full")) == 6075
    assert intra >= 100 and coded >= 1000 and skip >= 100, (intra, coded, skip)
