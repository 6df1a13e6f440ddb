"""The band deblocker's cut on the device (k_deblock.hip, "the cut"): the column each band of a P picture is cut at is a schedule decision that
does not change the output -- a wrong one is a race that comes out right on most runs -- so besides the output these tests pin the column
itself (Encoder.band_cuts(): the {cut, epoch} granule every band leaves) to tests/cutref.py's rule, check that it is safe, and that no bounded
wait ran out.  First crafted records through the single-stage deblocker, then content through the library's defaults."""
import numpy as np
import pytest

from tests import cutref
from tests.util import db_picture, first_diff, marked_records, random_records

pytestmark = pytest.mark.gpu

# (mbw, mbh): every width of the issue with every mbh % 4; 59 is below DB_CUT_MIN_MBW (bands walked whole); the widest rows the encoder opens for (512, 511) and the
# first past 256; 512 rows of the shortest row that is cut: 128 bands, all cut
SIZES = [(59, 9), (60, 12), (64, 13), (80, 14), (120, 15), (124, 11), (240, 21), (256, 10), (512, 5), (511, 8), (257, 4), (60, 512)]
SETTINGS = [(0, 0), (2, 4), (2, 8), (2, 20)]  # (disable_deblocking_filter_idc, slice rows)


def _chain_maps(mbw, mbh, seed):
    """Band by band through the branches of the choice: free only at the target, at the window's first or last column, nowhere, an idle
    band, free only left of the target, two columns around it -- in an order that changes with the seed, so that each branch meets bounds
    from different bands above."""
    first, last, tgt = cutref.window(mbw)
    specs = [{tgt}, {first}, {last}, set(), None, {first, (first + tgt) // 2}, {tgt - 3, tgt + 3}, {last - 1, tgt + 1}]
    nb = cutref.n_bands(mbh)
    win = set(range(first, last + 1))
    bands = []
    for b in range(nb):
        s = specs[(b * (seed + 1) + seed) % len(specs)]
        bands.append(None if s is None else win - s)
    return [marked_records(mbw, mbh, bands, t8=bool(seed & 1), qp=24 + 7 * seed)]


def _random_maps(mbw, mbh, seed):
    dense = random_records(mbw, mbh, seed=seed)
    sparse = random_records(mbw, mbh, seed=seed + 77, coded=0.04, intra=0.01, t8=0.5)
    g = np.random.Generator(np.random.PCG64(seed))
    still = g.random(sparse.size) < 0.9
    sparse["mvx"][still], sparse["mvy"][still] = 20, -8
    return [dense, sparse]


def _deblock_and_check(E, oracle, e, rec, idc, rows, seed, last_epoch):
    mbw, mbh = e.mbw, e.mbh
    y, uv = db_picture(mbw, mbh, seed)
    oracle.set_slice_rows(rows)
    oracle.set_slice_deblock(idc)
    try:
        want_y, want_uv = oracle.deblock_frame(y, uv, rec)
    finally:
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)
    got_y, got_uv = e.stage_deblock(y, uv, rec)
    assert np.array_equal(got_y, want_y), ("luma", first_diff(got_y, want_y))
    assert np.array_equal(got_uv, want_uv), ("chroma", first_diff(got_uv, want_uv))
    assert e.error_word() == 0, hex(e.error_word())
    bc = e.band_cuts()
    if mbw < cutref.DB_CUT_MIN_MBW:
        assert not bc["count"].any() and not bc["cut"].any() and not bc["epoch"].any(), "rows under DB_CUT_MIN_MBW are walked whole"
        return last_epoch, want_y
    cut = bc["cut"]
    exp = cutref.expected_cuts(rec, mbw, mbh, rows, idc)
    bad = np.argwhere(cut != exp)
    assert len(bad) == 0, ("first differing band, plane", tuple(bad[0]), "kernel", int(cut[tuple(bad[0])]), "reference", int(exp[tuple(bad[0])]))
    ep = np.unique(bc["epoch"])
    assert len(ep) == 1 and int(ep[0]) != last_epoch, ("every granule is this launch's", bc["epoch"])
    assert (bc["count"] % 2 == 0).all()
    for plane in range(2):
        for b in range(len(cut)):
            assert cutref.cut_is_safe(rec, mbw, mbh, b, int(cut[b, plane])), (b, plane, int(cut[b, plane]))
        assert cutref.never_steps_left(cut[:, plane], mbw, mbh, rows, idc) is None
    return int(ep[0]), want_y


@pytest.mark.parametrize("mbw,mbh", SIZES)
def test_crafted_records_cut_where_the_rule_says(E, oracle, mbw, mbh):
    """stage_deblock on crafted records and a picture that filters visibly, with idc 0 and with slice-local deblocking in slices of 4, 8 and
    20 rows: output equal to the oracle's in both planes; the column of every band and plane equal to the reference's, safe, never left of
    the band above's in a slice; every granule of this launch; no bounded wait ran out."""
    e = E.Encoder(16 * mbw, 16 * mbh, fixed_qp=30)
    epoch = 0
    try:
        for idc, rows in SETTINGS:
            if rows >= mbh:
                continue
            e.stage_set_slice_deblock(idc)
            e.stage_set_slice_rows(rows)
            for seed in range(3):
                for rec in _chain_maps(mbw, mbh, seed) + _random_maps(mbw, mbh, 100 * seed + rows + idc):
                    epoch, _ = _deblock_and_check(E, oracle, e, rec, idc, rows, seed + mbw, epoch)
        assert e.stats().recoveries == 0
    finally:
        e.close()


def test_crafted_records_reach_every_branch():
    """The maps above (taken on the reference, per width) reach every branch of the choice -- that the device agrees on them is the test above."""
    seen = set()
    for mbw, mbh in SIZES[1:]:
        for idc, rows in SETTINGS:
            if rows >= mbh:
                continue
            for seed in range(3):
                for rec in _chain_maps(mbw, mbh, seed):
                    _, why = cutref.expected_cuts(rec, mbw, mbh, rows, idc, trace=True)
                    for t in why:
                        seen.add(t["branch"])
                        if t.get("forced_right"):
                            seen.add("forced_right")
                        if t.get("forced_none"):
                            seen.add("forced_none")
                        if t["work"] and t["above"] in ("whole", "idle"):
                            seen.add("under_" + t["above"])
    assert {"idle", "none", "inner", "edge_left", "edge_right", "forced_right", "forced_none", "under_whole", "under_idle"} <= seen, seen


@pytest.mark.parametrize("mbw,mbh", SIZES)
def test_bands_walked_whole_give_the_same_output(E, oracle, monkeypatch, mbw, mbh):
    """MI355ENC_NO_SPLIT (read when an encoder is opened): the same records through bands walked whole -- a second implementation of the
    same output -- equal to the cut bands' and the oracle's; no granules are kept."""
    rec = random_records(mbw, mbh, seed=mbw, coded=0.05, intra=0.02)
    e = E.Encoder(16 * mbw, 16 * mbh, fixed_qp=30)
    try:
        e.stage_set_slice_deblock(2)
        e.stage_set_slice_rows(8)
        _, cut_y = _deblock_and_check(E, oracle, e, rec, 2, 8, 5, 0)
    finally:
        e.close()
    monkeypatch.setenv("MI355ENC_NO_SPLIT", "1")
    w = E.Encoder(16 * mbw, 16 * mbh, fixed_qp=30)
    try:
        w.stage_set_slice_deblock(2)
        w.stage_set_slice_rows(8)
        y, uv = db_picture(mbw, mbh, 5)
        whole_y, _ = w.stage_deblock(y, uv, rec)
        assert np.array_equal(whole_y, cut_y), first_diff(whole_y, cut_y)
        assert w.band_cuts() is None and w.error_word() == 0
    finally:
        w.close()


@pytest.mark.parametrize("first", ["rows", "idc"])
def test_slice_seams_inside_a_band_are_refused(E, first):
    """Slice-local deblocking needs slices of whole bands (four rows): idc 2 with slice rows that are not a multiple of four is refused by the
    single-stage calls (MI355ENC_ERR_ARG), whichever setting came first; idc 0 takes any rows, and a legal pair works again afterwards."""
    mbw, mbh = 64, 12
    e = E.Encoder(16 * mbw, 16 * mbh, fixed_qp=30)
    y, uv = db_picture(mbw, mbh, 1)
    rec = random_records(mbw, mbh, seed=1)
    try:
        if first == "rows":
            e.stage_set_slice_rows(6)
            e.stage_set_slice_deblock(2)
        else:
            e.stage_set_slice_deblock(2)
            e.stage_set_slice_rows(6)
        with pytest.raises(E.EncoderError, match=r"\(%d\)" % E.ERR_ARG):
            e.stage_deblock(y, uv, rec)
        e.stage_set_slice_deblock(0)
        e.stage_deblock(y, uv, rec)
        e.stage_set_slice_deblock(2)
        e.stage_set_slice_rows(8)
        e.stage_deblock(y, uv, rec)
        assert e.error_word() == 0
    finally:
        e.close()


# ---------------------------------------------------------------- content through the shipped configuration

def _content_run(E, oracle, kind, w, h, n, depth, tools, check_cuts):
    from tests.util import content_clip
    t8 = tools == "preset2"
    oracle.set_transform8x8(t8)
    oracle.set_i8x8(t8)
    try:
        e = E.Encoder(w, h, gop=30, fixed_qp=30, pipeline_depth=depth, exclusive=depth > 0, slices=None, slice_deblock=None, scenecut=False,
                      transform8x8=t8, i8x8=t8, aq=t8)
        mbh = (h + 15) // 16
        ns = oracle.auto_slices(mbh)
        oe = oracle.Encoder(w, h, gop=30, threads=16, intra_slices=0, p_slices=ns, slice_deblock_local=True, scenecut=False, aq=t8)
        dec = oracle.Decoder()
        rows = e.p_slice_rows
        assert rows == oracle.slice_rows_for(mbh, ns, True)
        clip = content_clip(kind, w, h, n)
        got, branches, prev = [], set(), None
        for i, (y, uv) in enumerate(clip):
            e.submit(y, uv, pts=i)
            if depth == 0:
                au, key = e.collect()[:2]
                ref_au, ref_key = oe.encode(y, uv, 30)
                assert au == ref_au and key == ref_key, ("bitstream", i)
                assert np.array_equal(e.fetch(E.FETCH_RECON_Y), oe.recon_y), ("recon", i)
                dy, duv = dec.decode(au)
                assert np.array_equal(dy, oe.recon_y) and np.array_equal(duv, oe.recon_uv), ("decoder", i)
                if check_cuts and not key:
                    bc = e.band_cuts()
                    assert prev is None or int(bc["epoch"][0, 0]) != prev, "a new launch with the cut for every P picture"
                    prev = int(bc["epoch"][0, 0])
                    assert len(np.unique(bc["epoch"])) == 1 and (bc["count"] % 2 == 0).all()
                    exp, why = cutref.expected_cuts(oe.mbinfo, e.mbw, e.mbh, rows, 2, trace=True)
                    bad = np.argwhere(bc["cut"] != exp)
                    assert len(bad) == 0, (i, "first differing band, plane", tuple(bad[0]), int(bc["cut"][tuple(bad[0])]), int(exp[tuple(bad[0])]))
                    for b in range(len(exp)):
                        assert cutref.cut_is_safe(oe.mbinfo, e.mbw, e.mbh, b, int(bc["cut"][b, 0]))
                    branches.update(t["branch"] for t in why)
                got.append(au)
            elif e.pending > depth:
                got.append(e.collect()[0])
        while e.pending:
            got.append(e.collect()[0])
        st = e.stats()
        assert st.recoveries == 0 and st.last_error_word == 0 and e.error_word() == 0
        e.close()
        return got, branches
    finally:
        oracle.set_transform8x8(False)
        oracle.set_i8x8(False)


CONTENT = ["s1", "s4pan", "s3", "flash", "letterbox", "strips"]


@pytest.mark.parametrize("tools", ["base", "preset2"])
@pytest.mark.parametrize("w,h,n", [(1280, 720, 5), (1920, 1080, 4)])
@pytest.mark.parametrize("kind", CONTENT)
def test_content_at_library_defaults_cut_where_the_rule_says(E, oracle, kind, w, h, n, tools):
    """Library defaults (sliced P pictures, slice-local deblocking), with the preset-2 toolset (8x8 transform, Intra_8x8, adaptive quantisation)
    and without: at depth 0 every picture's access unit, reconstruction and the decoder's picture equal the oracle's and every P picture's band
    columns equal the reference's on the oracle's records; at depth 2 (exclusive) the same stream without a recovery."""
    s0, branches = _content_run(E, oracle, kind, w, h, n, 0, tools, True)
    s2, _ = _content_run(E, oracle, kind, w, h, n, 2, tools, False)
    assert s2 == s0
    if kind == "strips":
        assert {"edge_left", "edge_right", "none", "idle"} <= branches, branches
    if kind == "s3":
        assert branches <= {"none"}, branches
    if kind == "letterbox":
        assert "idle" in branches


@pytest.mark.parametrize("kind", ["strips", "flash"])
def test_content_at_2160p_cut_where_the_rule_says(E, oracle, kind):
    s0, _ = _content_run(E, oracle, kind, 3840, 2160, 3, 0, "base", True)
    s2, _ = _content_run(E, oracle, kind, 3840, 2160, 3, 2, "base", False)
    assert s2 == s0


def _n_slices(au):
    """coded slices of a non-IDR picture in an access unit (NAL unit type 1)"""
    return sum(1 for k in range(len(au) - 3) if au[k:k + 3] == b"\x00\x00\x01" and au[k + 3] & 0x1F == 1)


@pytest.mark.parametrize("depth", [0, 2])
def test_drop_ladder_at_library_defaults(E, oracle, depth):
    """The drop ladder and all-skip plan of test_drop_ladder_and_all_skip_pictures_equal_oracle at library defaults, 1080p: an all-skip picture is
    written as one slice between sliced pictures, the stream is the oracle's, and (depth 0) the band columns of every P picture after one are
    still the rule's."""
    from tests.util import frames
    w, h = 1920, 1080
    plan = [(40, 0), (51, 0), (51, 2), (51, 255), (51, 255), (51, 5), (46, 0), (51, 255), (30, 0)]
    e = E.Encoder(w, h, gop=30, fixed_qp=40, pipeline_depth=depth, exclusive=depth > 0, keep_prefilter=True, slices=None, slice_deblock=None, scenecut=False)
    mbh = (h + 15) // 16
    ns = oracle.auto_slices(mbh)
    oe = oracle.Encoder(w, h, gop=30, threads=16, intra_slices=0, p_slices=ns, slice_deblock_local=True, scenecut=False)
    dec = oracle.Decoder()
    rows = e.p_slice_rows
    assert rows > 0
    clip = [(y, uv) for _, _, y, uv in frames(w, h, len(plan))]
    got, cuts_checked = [], 0
    for i, (y, uv) in enumerate(clip):
        qp, drop = plan[i]
        e.set_fixed_qp(qp)
        e.set_fixed_drop(drop)
        e.submit(y, uv, pts=i)
        if depth == 0:
            got.append(e.collect() + (e.last_drop,))
            ref_au, ref_key = oe.encode(y, uv, qp, drop=drop)
            got[-1] += (ref_au, ref_key, oe.recon_y.copy(), oe.recon_uv.copy())
            if not ref_key and drop != 255:
                bc = e.band_cuts()
                exp = cutref.expected_cuts(oe.mbinfo, e.mbw, e.mbh, rows, 2)
                assert np.array_equal(bc["cut"], exp), (i, first_diff(bc["cut"], exp))
                cuts_checked += 1
        elif e.pending > depth:
            got.append(e.collect() + (e.last_drop,))
    while e.pending:
        got.append(e.collect() + (e.last_drop,))
    if depth == 0:
        assert cuts_checked == 5  # every P picture of the plan but the three all-skip ones
    for i, (y, uv) in enumerate(clip):
        qp, drop = plan[i]
        if depth == 0:
            au, key, pts, gqp, gdrop, ref_au, ref_key, ry, ruv = got[i]
        else:
            au, key, pts, gqp, gdrop = got[i]
            ref_au, ref_key = oe.encode(y, uv, qp, drop=drop)
            ry, ruv = oe.recon_y, oe.recon_uv
        assert (key, pts, gqp, gdrop) == (ref_key, i, qp, drop) and au == ref_au, ("bitstream", i)
        if drop == 255:
            assert len(au) < 40 and _n_slices(au) == 1, "an all-skip picture is one slice"
        elif not key:
            assert _n_slices(au) == (mbh + rows - 1) // rows, "the sliced pictures around it"
        dy, duv = dec.decode(au)
        assert np.array_equal(dy, ry) and np.array_equal(duv, ruv), i
    st = e.stats()
    assert st.recoveries == 0 and e.error_word() == 0
    e.close()
