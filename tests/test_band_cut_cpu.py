"""The band deblocker's cut without a device: tests/cutref.py (the rule, from 8.7.2.1 and DESIGN sections 4-5) pinned to the CPU oracle's
deblocking -- a column with bS = 0 in every row really splits the picture's filtering in two, a busy one does not -- and to hand-computed
columns for every branch of the choice; then the preconditions of the engineered content the GPU tests rely on."""
import numpy as np
import pytest

from tests import cutref
from tests.util import db_picture, free_column, marked_records, random_records, window_edge_pattern


@pytest.fixture
def one_slice(oracle):
    oracle.set_slice_rows(0)
    oracle.set_slice_deblock(0)
    yield oracle
    oracle.set_slice_rows(0)
    oracle.set_slice_deblock(0)


def _split_equals_whole(oracle, y, uv, rec, mbw, mbh, col):
    r = rec.reshape(mbh, mbw)
    wy, wuv = oracle.deblock_frame(y, uv, rec)
    ly, luv = oracle.deblock_frame(np.ascontiguousarray(y[:, :16 * col]), np.ascontiguousarray(uv[:, :16 * col]), np.ascontiguousarray(r[:, :col]).reshape(-1))
    ry, ruv = oracle.deblock_frame(np.ascontiguousarray(y[:, 16 * col:]), np.ascontiguousarray(uv[:, 16 * col:]), np.ascontiguousarray(r[:, col:]).reshape(-1))
    return np.array_equal(np.hstack([ly, ry]), wy) and np.array_equal(np.hstack([luv, ruv]), wuv)


# ---------------------------------------------------------------- the premise: a free column splits the filtering in two

@pytest.mark.parametrize("t8", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("qps", [(10, 51), (51, 10), (15, 16), (51, 51), (28, 40)])
def test_a_free_column_splits_the_picture_in_two(one_slice, t8, qps):
    """8.7: across a macroblock edge with bS = 0 in every row the filter reads and writes nothing, so deblocking the strips left and
    right of it on their own (the right strip's first column a picture edge) gives the whole picture's result -- luma and chroma, with
    and without the 8x8 transform, whatever the QPs on either side (QP < 16: alpha 0; 51)."""
    oracle = one_slice
    mbw, mbh, col = 24, 9, 11
    rec = random_records(mbw, mbh, seed=7 + int(10 * t8) + qps[0], t8=t8)
    r = rec.reshape(mbh, mbw)
    r[:, :col]["qp"] = qps[0]
    r[:, col:]["qp"] = qps[1]
    free_column(rec, mbw, mbh, col)
    assert not (cutref.vertical_mb_edge_bs(rec, mbw, mbh)[:, col] > 0).any()
    assert all(cutref.cut_is_safe(rec, mbw, mbh, b, col) for b in range(cutref.n_bands(mbh)))
    y, uv = db_picture(mbw, mbh, seed=3)
    wy, _ = oracle.deblock_frame(y, uv, rec)
    assert not np.array_equal(wy, y), "the picture filters visibly"
    assert _split_equals_whole(oracle, y, uv, rec, mbw, mbh, col)


@pytest.mark.parametrize("idc,rows", [(0, 0), (2, 4), (2, 8)])
def test_a_free_column_splits_the_picture_with_slices(oracle, idc, rows):
    """The same with slices: the strips are cut along the same slice rows, with disable_deblocking_filter_idc 0 and 2."""
    mbw, mbh, col = 20, 13, 9
    rec = free_column(random_records(mbw, mbh, seed=99 + rows), mbw, mbh, col)
    y, uv = db_picture(mbw, mbh, seed=4)
    oracle.set_slice_rows(rows)
    oracle.set_slice_deblock(idc)
    try:
        assert _split_equals_whole(oracle, y, uv, rec, mbw, mbh, col)
    finally:
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)


@pytest.mark.parametrize("kind", ["intra", "coded", "coded_t8", "mv4", "mvy5"])
def test_a_busy_column_does_not_split(one_slice, kind):
    """The converse, so that the premise test can fail: a column the reference calls busy (bS > 0 in some row), at a QP where the filter
    works, makes the split differ from the whole picture."""
    oracle = one_slice
    mbw, mbh, col = 24, 8, 10
    rec = free_column(random_records(mbw, mbh, seed=5, qp=(36, 44)), mbw, mbh, col)
    r = rec.reshape(mbh, mbw)
    y0 = 3
    if kind == "intra":
        r[y0, col]["mb_type"] = 0
    elif kind == "coded":
        r[y0, col - 1]["nzmask"] = int(r[y0, col - 1]["nzmask"]) | (1 << 15)            # blkIdx 15: raster (3, 3)
    elif kind == "coded_t8":
        r[y0, col]["nzmask"] = int(r[y0, col]["nzmask"]) | (1 << 27) | (1 << 9)          # 8x8 block 2 (raster rows 2, 3 of column 0)
    elif kind == "mv4":
        r[y0, col]["mvx"] = int(r[y0, col - 1]["mvx"]) + 4
    else:
        r[y0, col]["mvy"] = int(r[y0, col - 1]["mvy"]) - 5
    assert (cutref.vertical_mb_edge_bs(rec, mbw, mbh)[y0, col] > 0).any()
    assert not cutref.cut_is_safe(rec, mbw, mbh, y0 // 4, col)
    assert not _split_equals_whole(oracle, db_picture(mbw, mbh, seed=6)[0], db_picture(mbw, mbh, seed=6)[1], rec, mbw, mbh, col)


def test_mv_difference_of_three_is_free(one_slice):
    """bS 1 starts at a difference of 4 quarter samples: 3 leaves the edge alone, in either component."""
    mbw, mbh, col = 16, 4, 7
    rec = free_column(random_records(mbw, mbh, seed=11), mbw, mbh, col)
    r = rec.reshape(mbh, mbw)
    r[:, col]["mvx"] = r[:, col - 1]["mvx"] + 3
    r[:, col]["mvy"] = r[:, col - 1]["mvy"] - 3
    assert cutref.cut_is_safe(rec, mbw, mbh, 0, col)
    y, uv = db_picture(mbw, mbh, seed=8)
    assert _split_equals_whole(one_slice, y, uv, rec, mbw, mbh, col)


def test_reference_bs_agrees_with_the_oracle_filter(one_slice):
    """Every vertical macroblock edge of a random map: the oracle's filtering splits there exactly when the reference calls it free
    (given a picture that filters wherever bS > 0 lets it) -- the reference's bS is the oracle's, edge by edge, not only on crafted maps."""
    mbw, mbh = 14, 2
    rec = random_records(mbw, mbh, seed=21, qp=(38, 42), coded=0.15, intra=0.03)
    for col in (3, 9):
        free_column(rec, mbw, mbh, col, rows=[0])  # (row 1 as it comes)
    y, uv = db_picture(mbw, mbh, seed=9)
    free = ~(cutref.vertical_mb_edge_bs(rec, mbw, mbh) > 0).any(axis=(0, 2))
    assert 2 <= free[1:].sum() <= mbw - 3, free
    for col in range(1, mbw):
        assert _split_equals_whole(one_slice, y, uv, rec, mbw, mbh, col) == bool(free[col]), col


# ---------------------------------------------------------------- hand-computed columns for every branch of the choice

# (mbw, mbh, idc, slice_rows, per band: None = idle or the set of busy window columns (all others free), expected cut per band, branch per band)
def _busy_but(mbw, free):
    first, last, _ = cutref.window(mbw)
    return set(range(first, last + 1)) - set(free)


FIXTURES = {
    # mbw 60: window 15 .. 45, target 29
    "60_free_and_none": (60, 8, 0, 0, [set(), _busy_but(60, [])], [29, 60], ["inner", "none"]),
    # mbw 60, idc 2, every band a slice of its own (4 rows): no band keeps to the one above
    "60_slices_of_one_band": (60, 12, 2, 4, [_busy_but(60, [45]), _busy_but(60, [15, 30]), _busy_but(60, [20])], [45, 30, 20],
                              ["edge_right", "inner", "inner"]),
    # mbw 64: window 16 .. 48, target 30; mbh % 4 == 1 (last band one row).  Bit 32 of the mask: column 48
    "64_edges_bound_whole": (64, 13, 0, 0, [_busy_but(64, [16]), _busy_but(64, [48]), _busy_but(64, [30, 40]), _busy_but(64, [25])],
                             [16, 48, 64, 25], ["edge_left", "edge_right", "none", "inner"]),
    # mbw 120: window 30 .. 90, target 57; mbh % 4 == 2.  A cut right of the target at bit 35; an idle band; a band below it keeps to nothing
    "120_bound_idle": (120, 14, 0, 0, [_busy_but(120, [40, 75]), _busy_but(120, [45, 65]), None, _busy_but(120, [30, 58])],
                       [40, 65, 0, 58], ["inner", "inner", "idle", "inner"]),
    # mbw 120, equal distance: right first
    "120_tie_right_first": (120, 4, 0, 0, [_busy_but(120, [53, 61])], [61], ["inner"]),
    # mbw 124: window 31 .. 93, target 59; mbh % 4 == 3; idc 2, slices of 8 rows: band 2 is a slice's first under a cut far right
    "124_forced_right_then_slice_top": (124, 11, 2, 8, [_busy_but(124, [93]), _busy_but(124, [60, 90, 93]), _busy_but(124, [31, 60])],
                                        [93, 93, 60], ["edge_right", "edge_right", "inner"]),
    # ... the same records with idc 0: band 2 keeps to 93 and finds nothing right of it
    "124_same_idc0": (124, 11, 0, 8, [_busy_but(124, [93]), _busy_but(124, [60, 90, 93]), _busy_but(124, [31, 60])],
                      [93, 93, 124], ["edge_right", "edge_right", "none"]),
    # mbw 124, a whole band (no free column) above: nothing to keep to; then the bound at the window's left edge
    "124_under_whole": (124, 16, 0, 0, [_busy_but(124, []), _busy_but(124, [31, 100]), _busy_but(124, [31, 45]), None],
                        [124, 31, 45, 0], ["none", "edge_left", "inner", "idle"]),
}


@pytest.mark.parametrize("t8", [False, True])
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_expected_cuts_hand_computed(name, t8):
    mbw, mbh, idc, rows, bands, want, branches = FIXTURES[name]
    rec = marked_records(mbw, mbh, bands, t8=t8)
    assert list(cutref.band_work(rec, mbw, mbh, rows, idc)) == [b is not None for b in bands]
    cuts, why = cutref.expected_cuts(rec, mbw, mbh, rows, idc, trace=True)
    assert list(cuts[:, 0]) == want and list(cuts[:, 1]) == want, (name, cuts[:, 0])
    assert [t["branch"] for t in why] == branches, (name, why)
    for b, c in enumerate(want):
        assert cutref.cut_is_safe(rec, mbw, mbh, b, c)
    assert cutref.never_steps_left(cuts[:, 0], mbw, mbh, rows, idc) is None


def test_fixtures_reach_every_branch():
    """The fixtures above, taken together, reach each branch the issue of the cut lists (a count, not a rate)."""
    seen = set()
    for name, (mbw, mbh, idc, rows, bands, want, _) in FIXTURES.items():
        _, why = cutref.expected_cuts(marked_records(mbw, mbh, bands), mbw, mbh, rows, idc, trace=True)
        for t in why:
            seen.add(t["branch"])
            if t.get("forced_right"):
                seen.add("forced_right")
            if t.get("forced_none"):
                seen.add("forced_none")
            if t["work"] and t["above"] in ("whole", "idle"):
                seen.add("under_" + t["above"])
            if t["work"] and t["band"] > 0 and t["above"] is None and idc == 2:
                seen.add("slice_top")
        seen.update({"mbh%%4=%d" % (mbh % 4)})
    want = {"idle", "none", "inner", "edge_left", "edge_right", "forced_right", "forced_none", "under_whole", "under_idle", "slice_top",
            "mbh%4=0", "mbh%4=1", "mbh%4=2", "mbh%4=3"}
    assert want <= seen, want - seen


def test_window_geometry():
    """cut_w = min(mbw / 4, 31): the mask never needs more than 63 bits; the window's last column is bit 32 or more from mbw 64 on."""
    for mbw in range(60, 300):
        first, last, tgt = cutref.window(mbw)
        assert 0 < first < tgt <= mbw // 2 < last < mbw and last - first <= 62
    assert cutref.window(60) == (15, 45, 29) and cutref.window(64) == (16, 48, 30)
    assert cutref.window(120) == (30, 90, 57) and cutref.window(124) == (31, 93, 59) and cutref.window(256) == (97, 159, 125)


def test_reference_on_random_maps_is_safe_and_ordered():
    """Seeded random maps at the GPU tests' widths: every chosen column is safe, none steps left inside a slice, both planes agree."""
    for mbw in (60, 64, 80, 120, 124, 240, 256):
        for mbh, idc, rows in ((17, 0, 0), (22, 2, 8), (30, 2, 20), (13, 2, 4)):
            for seed in range(3):
                rec = random_records(mbw, mbh, seed=seed * 1000 + mbw, coded=0.05, intra=0.01, t8=0.5)
                cuts = cutref.expected_cuts(rec, mbw, mbh, rows, idc)
                for b in range(len(cuts)):
                    assert cutref.cut_is_safe(rec, mbw, mbh, b, int(cuts[b, 0]))
                assert cutref.never_steps_left(cuts[:, 0], mbw, mbh, rows, idc) is None


# ---------------------------------------------------------------- preconditions of the engineered content (GPU: tests/test_band_cut_gpu.py)

@pytest.mark.parametrize("w,h", [(1280, 720), (1920, 1080)])
def test_window_edge_strips_steer_the_cut(oracle, w, h):
    """The noise-strip clip at library defaults (oracle records of its P pictures): bands choose the window's left edge, its right edge
    (at 1080p column 90: bit 60, the mask's second word) and no column at all, some bands are idle, some keep to a cut of the band
    above and some to nothing below an idle or a whole band.  So a GPU failure on this clip is the kernel's, not the content's."""
    from tests.util import noise_strip_clip
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    ns = oracle.auto_slices(mbh)
    rows = oracle.slice_rows_for(mbh, ns, True)
    oe = oracle.Encoder(w, h, gop=60, threads=16, intra_slices=0, p_slices=ns, slice_deblock_local=True, scenecut=False)
    first, last, _ = cutref.window(mbw)
    seen = set()
    for i, (y, uv) in enumerate(noise_strip_clip(w, h, 3, window_edge_pattern)):
        oe.encode(y, uv, 30)
        if i == 0:
            continue
        cuts, why = cutref.expected_cuts(oe.mbinfo, mbw, mbh, rows, 2, trace=True)
        for t in why:
            seen.add(t["branch"])
            if t["work"] and t["above"] in ("whole", "idle"):
                seen.add("under_" + t["above"])
            if t["bound"] is not None:
                seen.add("bound")
        assert set(cuts[:, 0].tolist()) <= {0, first, last, mbw}, cuts[:, 0]
    oe.close()
    assert {"edge_left", "edge_right", "none", "idle", "under_whole", "under_idle", "bound"} <= seen, seen
    if mbw == 120:
        assert last - first == 60
