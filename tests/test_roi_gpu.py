"""GPU: region-of-interest quantisation.  The compose launch against clamp(orc_aq_offsets + t); the intra and the fused P stage under
a map against the oracle's stage functions under orc_set_aq_map (tests/roiref.py: the composed pictures the CPU tests decode); whole streams whose map changes
with every picture while earlier pictures are in flight -- every access unit through the oracle's decoder, QP_Y of every macroblock that sends a delta against
that picture's own map, the first IDR picture under a map against the composed oracle byte for byte, and a stream of inactive maps against oracle.Encoder's
byte for byte; what the schedule books for pictures with and without offsets; and the direction the bits move in."""
import functools

import numpy as np
import pytest

from tests import roiref as R
from tests import t8ref
from tests.util import first_diff, frames

pytestmark = pytest.mark.gpu

FIELDS = ("mvx", "mvy", "mb_type", "i16_mode", "chroma_mode", "nzmask", "cost")


# ---------------------------------------------------------------- the compose launch
@pytest.mark.parametrize("aq", [False, True])
@pytest.mark.parametrize("w,h", [(64, 48), (80, 48), (322, 182), (720, 400)])
def test_offsets_are_the_aq_offsets_moved_by_the_map(E, oracle, w, h, aq):
    """64 x 48: twelve macroblocks, whole words; 80 x 48: fifteen, the byte tail; 322 x 182: a partly padded last row and column under aq_kernel; 720 x 400:
    1125 macroblocks, more than one workgroup of 1024 and a tail of one"""
    yp = frames(w, h, 1)[0][0]
    e = E.Encoder(w, h, fixed_qp=30, aq=aq)
    try:
        mbw, mbh = e.mbw, e.mbh
        assert e.debug_roi_bytes() == 0 and e.get_roi() is None
        assert np.array_equal(e.roi_probe_offsets(yp), R.offsets(oracle, yp, np.zeros((mbh, mbw)), aq))  # no map: the aq offsets alone (zeros without)
        cfg = dict(rects=[(w // 4, h // 4, w // 2, h // 2, -12, 2), (0, 0, 24, 24, 12, 1), (w - 20, h - 20, 64, 64, 7, 0)], balance=4)
        user = np.random.default_rng(w).integers(-4, 5, (mbh, mbw)).astype(np.int8)
        user[-1, -1] = -12  # (the last macroblock: the tail's last byte)
        t = R.roi_map(cfg, user, mbw, mbh)[0]
        e.set_roi(cfg, user)
        assert e.get_roi() == dict(rects=[tuple(r) for r in cfg["rects"]], balance=4)
        got = e.roi_probe_offsets(yp)
        want = R.offsets(oracle, yp, t, aq)
        assert np.array_equal(got, want), first_diff(got, want)
        assert t.min() == -12 and len(np.unique(want)) > 3
        if aq:
            assert (R.aq_offsets(oracle, yp) != 0).any() and not np.array_equal(want, t)  # the composition is no copy of either part
        assert e.debug_roi_bytes() == (0 if aq else 3 * (mbw * mbh + 16))
        e.set_roi(dict(rects=[], balance=6), np.zeros((mbh, mbw), np.int8))  # an inactive map is no map
        assert np.array_equal(e.roi_probe_offsets(yp), R.offsets(oracle, yp, np.zeros((mbh, mbw)), aq))
        e.set_roi(None)
        assert e.get_roi() is None
    finally:
        e.close()


# ---------------------------------------------------------------- single stages under a map
def _records_equal(got, want, where=""):
    for f in FIELDS:
        assert np.array_equal(got[f], want[f]), (where, f, first_diff(got[f], want[f]))
    sent = R.sends_delta(want)
    assert np.array_equal(got["qp"][sent], want["qp"][sent]), (where, "qp")  # (the qp byte only where a delta is sent: include/mi355enc.h, MI355ENC_FETCH_MBINFO)


def _picture_equal(got, want, where=""):
    rec_y, rec_uv, mbi, lev = got
    wy, wuv, wmbi, wlev = want
    _records_equal(mbi, wmbi, where)
    assert np.array_equal(lev, wlev), (where, "levels", first_diff(lev, wlev))
    assert np.array_equal(rec_y, wy) and np.array_equal(rec_uv, wuv), (where, "reconstruction", first_diff(rec_y, wy))


@pytest.mark.parametrize("qp", R.QPS_COMPOSED)
@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("w,h", R.SIZES_COMPOSED)
def test_stages_under_a_map_equal_the_oracle(E, oracle, w, h, slices, qp):
    """mi355enc_stage_intra and mi355enc_stage_pmb with run_intra_p under mi355enc_roi_probe_set_map(t) against orc_intra_frame and orc_pmb_frame +
    orc_intra_p_frame under orc_set_aq_map(t): records, levels and reconstruction; with the map cleared again the stages give today's result"""
    c = R.composed(w, h, slices, qp)
    (y0, uv0), (y1, uv1) = c["clip"][0][:2], c["clip"][1][:2]
    idr, p, t = c["idr"], c["p"], c["t"]
    e = E.Encoder(w, h, fixed_qp=qp)
    try:
        e.stage_set_slice_rows(c["rows"])
        oracle.set_slice_rows(c["rows"])
        plain_i = e.stage_intra(y0, uv0, qp)
        plain_p = e.stage_pmb(y1, uv1, idr["rec_y"], idr["rec_uv"], p["imv"], oracle.surf_to_device(p["surf"]), qp, idec=p["idec"], run_intra_p=True)
        _picture_equal(plain_i, oracle.intra_frame(y0, uv0, qp), "intra, no map")
        e.roi_probe_set_map(t)
        got = e.stage_intra(y0, uv0, qp)
        py, puv, pmbi = idr["pre"]
        _picture_equal(got, (py, puv, pmbi, idr["lev"]), "intra")
        assert not np.array_equal(got[0], plain_i[0])
        got = e.stage_pmb(y1, uv1, idr["rec_y"], idr["rec_uv"], p["imv"], oracle.surf_to_device(p["surf"]), qp, idec=p["idec"], run_intra_p=True)
        py, puv, pmbi = p["pre"]
        _picture_equal(got, (py, puv, pmbi, p["lev"]), "pmb + intra_p")
        e.roi_probe_set_map(None)
        for a, b in zip(e.stage_intra(y0, uv0, qp) + e.stage_pmb(y1, uv1, idr["rec_y"], idr["rec_uv"], p["imv"], oracle.surf_to_device(p["surf"]), qp, idec=p["idec"], run_intra_p=True),
                        plain_i + plain_p):
            assert np.array_equal(a, b)
        with pytest.raises(E.EncoderError):
            e.roi_probe_set_map(np.full((e.mbh, e.mbw), 13, np.int8))
    finally:
        oracle.set_slice_rows(0)
        e.close()


def _mb_out(res, n, mbw):
    rec_y, rec_uv, mbi, lev = res
    mby, mbx = divmod(n, mbw)
    return (mbi[n].tobytes(), lev[n].tobytes(), rec_y[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16].tobytes(), rec_uv[8 * mby:8 * mby + 8, 16 * mbx:16 * mbx + 16].tobytes())


@pytest.mark.parametrize("qp", R.QPS_COMPOSED)
@pytest.mark.parametrize("w,h", R.SIZES_COMPOSED)
def test_stages_under_a_map_with_the_8x8_toolset(E, oracle, w, h, qp):
    """transform8x8 2 with i8x8: the intra stage against orc_intra_frame with the 8x8 transform and Intra_8x8 under the map; the fused P stage with the fixed
    8x8 transform (transform8x8 1) against orc_pmb_frame under the map, and the adaptive one (2) as the splice of the two fixed ones by the rule of
    tests/t8ref.py -- which is how the oracle reaches mode 2 (tests/test_t8_adaptive_gpu.py) -- macroblocks independent (no intra pass)"""
    c = R.composed(w, h, 1, qp)
    (y0, uv0), (y1, uv1) = c["clip"][0][:2], c["clip"][1][:2]
    idr, p, t = c["idr"], c["p"], c["t"]
    mbw = y0.shape[1] // 16
    surf = oracle.surf_to_device(p["surf"])
    res = {}
    oracle.set_transform8x8(True)
    oracle.set_i8x8(True)
    R.set_aq_map(oracle, t)
    try:
        want_i = oracle.intra_frame(y0, uv0, qp)
        full_p = oracle.pmb_frame(y1, uv1, idr["rec_y"], idr["rec_uv"], p["imv"], p["surf"], qp, idec=p["idec"], threads=8)
        want_p, want_lev = full_p[4], full_p[3]  # (records and reconstruction before the intra pass; the levels of inter macroblocks are final)
    finally:
        R.set_aq_map(oracle, None)
        oracle.set_i8x8(False)
        oracle.set_transform8x8(False)
    for mode in (0, 1, 2):
        e = E.Encoder(w, h, fixed_qp=qp, transform8x8=mode, i8x8=mode == 2)
        try:
            e.roi_probe_set_map(t)
            if mode == 2:
                _picture_equal(e.stage_intra(y0, uv0, qp), want_i, "intra, i8x8")
                if qp <= 37:
                    assert (want_i[2]["nzmask"] & (1 << 27)).any(), "no Intra_8x8 macroblock under the map"
            res[mode] = e.stage_pmb(y1, uv1, idr["rec_y"], idr["rec_uv"], p["imv"], surf, qp, idec=p["idec"], run_intra_p=False)
        finally:
            e.close()
    # the fixed 8x8 transform against the oracle, on the macroblocks the stage codes itself (those decided intra wait for the intra pass)
    inter = want_p[0]["mb_type"] == 1
    assert np.array_equal(res[1][2]["mb_type"] == 1, inter) and inter.any() and (want_p[0]["nzmask"][inter] & (1 << 27)).any()
    _records_equal(res[1][2][inter], want_p[0][inter], "pmb, 8x8")
    assert np.array_equal(res[1][3][inter], want_lev[inter])
    luma = np.repeat(np.repeat(inter.reshape(-1, mbw), 16, 0), 16, 1)
    assert np.array_equal(res[1][0][luma], want_p[1][luma]) and np.array_equal(res[1][1][luma[::2]], want_p[2][luma[::2]])
    for n in range(res[0][2].size):
        o0, o1, o2 = _mb_out(res[0], n, mbw), _mb_out(res[1], n, mbw), _mb_out(res[2], n, mbw)
        if o0 == o1:
            assert o2 == o0, n
            continue
        mby, mbx = divmod(n, mbw)
        use8 = t8ref.decide(y1, idr["rec_y"], mbx, mby, int(res[2][2]["mvx"][n]), int(res[2][2]["mvy"][n]))
        assert o2 == (o1 if use8 else o0), (n, use8)


# ---------------------------------------------------------------- whole streams
NPIC, GOP, QP = 8, 4, 30
SLICINGS = {"library": (dict(slices=None, slice_deblock=None), None), "one": (dict(slices=1, intra_slices=1, slice_deblock=False), dict(intra_slices=1, p_slices=1)),
            "two": (dict(slices=2, intra_slices=2, slice_deblock=True), dict(intra_slices=2, p_slices=2, slice_deblock_local=True))}


@functools.lru_cache(maxsize=None)
def _clip(w, h):
    return frames(w, h, NPIC)


def _maps(w, h):
    """per picture (cfg, user) -- None: set_roi(None); the map changes with (nearly) every picture: none, A, A, A moved, user map + balance, none, none, B"""
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    A = dict(rects=[(w // 4, h // 4, w // 3, h // 3, -6, 2)], balance=0)
    A2 = dict(rects=[(w // 4 + 48, h // 4 + 16, w // 3, h // 3, -6, 2)], balance=0)
    user = np.zeros((mbh, mbw), np.int8)
    user[mbh // 3:2 * mbh // 3, mbw // 3:2 * mbw // 3] = -5
    user[0, :] = 3
    Bc = dict(rects=[(0, 0, 64, 64, 5, 1), (w // 2, h // 2, 100, 60, -12, 3)], balance=3)
    return [None, (A, None), (A, None), (A2, None), (dict(rects=[], balance=6), user), None, None, (Bc, None)]


def _okw(oracle, slicing, mbh):
    return SLICINGS[slicing][1] or dict(intra_slices=0, p_slices=oracle.auto_slices(mbh), slice_deblock_local=True)


def _run_stream(E, e, clip, maps, depth):
    """submit with the picture's map set immediately before, earlier pictures still in flight -> [(au, key, last_roi, recon at depth 0)]"""
    got = []

    def collect():
        au, key, _ = e.collect()[:3]
        got.append((au, key, e.last_roi(), (e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)) if depth == 0 or not e.pending else None))

    for i, (_, _, y, uv) in enumerate(clip):
        if maps[i] is None:
            e.set_roi(None)
        else:
            e.set_roi(*maps[i])
        e.submit(y, uv, pts=i)
        if e.pending > depth:
            collect()
    while e.pending:
        collect()
    return got


@pytest.mark.parametrize("aq", [False, True])
@pytest.mark.parametrize("depth", [0, 2])
@pytest.mark.parametrize("slicing", ["library", "one", "two"])
@pytest.mark.parametrize("w,h", [(322, 182), (640, 368)])
def test_streams_whose_map_changes_with_every_picture(E, oracle, w, h, slicing, depth, aq):
    clip, maps = _clip(w, h), _maps(w, h)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    want_t = [(np.zeros((mbh, mbw), np.int8), False, 0) if m is None else R.roi_map(m[0], m[1], mbw, mbh) for m in maps]
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, exclusive=True, aq=aq, scenecut=False, **SLICINGS[slicing][0])
    oe = oracle.Encoder(w, h, gop=GOP, threads=8, aq=aq, scenecut=False, **_okw(oracle, slicing, mbh))
    dec = oracle.Decoder()
    try:
        c1 = e.debug_get_counters()
        got = _run_stream(E, e, clip, maps, depth)
        c2, st = e.debug_get_counters(), e.stats()
        assert [g[1] for g in got] == [i % GOP == 0 for i in range(NPIC)]
        with_off = [aq or want_t[i][1] for i in range(NPIC)]
        for i, (au, key, last, rec) in enumerate(got):
            t, active, bg = want_t[i]
            assert last == (active, bg if active else 0, int(t.astype(np.int64).sum()) if active else 0), (i, last)
            cap, _ = dec.capture(mbw * mbh)
            dy, duv = dec.decode(au)
            if rec is not None:
                assert np.array_equal(dy, rec[0]) and np.array_equal(duv, rec[1]), ("decoded picture", i)
            rows = e.slice_rows if key else e.p_slice_rows
            off = R.offsets(oracle, clip[i][0], t, aq)
            deltas = R.check_qp(cap, cap["qp"], QP, off if with_off[i] else np.zeros_like(off), mbw, rows)
            if active:
                assert deltas.size and np.abs(deltas).max() > 0, ("no delta under an active map", i)
            if i == 0:  # in front of the first active map: oracle.Encoder's stream
                assert au == oe.encode(clip[0][2], clip[0][3], QP)[0]
            if i == GOP:  # the first IDR picture under a map: the composed oracle, byte for byte
                d2 = oracle.Decoder()
                ref = R.compose_idr(oracle, d2, w, h, clip[i][0], clip[i][1], QP, off, rows, 0 if slicing == "one" else 2, idr_pic_id=1)
                d2.close()
                assert au == ref["au"], ("the IDR picture under a map", len(au), len(ref["au"]))
                assert rec is None or np.array_equal(rec[0], ref["rec_y"])
        # bookings: the QP_Y chain rode in the band launch of exactly the pictures with offsets (tests/test_longrun_gpu.py::_bookings)
        assert (c2["qpc_total"] - c1["qpc_total"]) & 0xFFFFFFFF == mbh * sum(with_off), (c1, c2, with_off)
        assert st.recoveries == 0 and st.last_error_word == 0 and e.error_word() == 0
        assert e.debug_roi_bytes() == (0 if aq else 3 * (mbw * mbh + 16))
    finally:
        e.close(); oe.close(); dec.close()


@pytest.mark.parametrize("aq", [False, True])
@pytest.mark.parametrize("depth", [0, 2])
def test_a_stream_of_inactive_maps_is_the_oracle_encoders(E, oracle, depth, aq):
    """every set_roi carries a map that says nothing -- no rectangle, a rectangle outside the picture, a caller's map of zeros, a balance with nothing to
    balance: the stream is oracle.Encoder's byte for byte, nothing was allocated, no QP_Y chain was booked that aq_mode does not book"""
    w, h = 322, 182
    clip = _clip(w, h)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    zero = np.zeros((mbh, mbw), np.int8)
    maps = [(dict(rects=[], balance=0), None), (None, zero), (dict(rects=[(-64, 0, 64, 64, -6, 8)], balance=6), None), (dict(rects=[], balance=12), zero)] * 2
    e = E.Encoder(w, h, gop=GOP, fixed_qp=QP, pipeline_depth=depth, exclusive=True, aq=aq, scenecut=False, slices=None, slice_deblock=None)
    oe = oracle.Encoder(w, h, gop=GOP, threads=8, aq=aq, scenecut=False, **_okw(oracle, "library", mbh))
    try:
        c1 = e.debug_get_counters()
        got = _run_stream(E, e, clip, maps, depth)
        c2 = e.debug_get_counters()
        for i, (au, key, last, rec) in enumerate(got):
            assert au == oe.encode(clip[i][2], clip[i][3], QP)[0], i
            assert last == (False, 0, 0)
        assert np.array_equal(got[-1][3][0], oe.recon_y)
        assert e.debug_roi_bytes() == 0 and (c2["qpc_total"] - c1["qpc_total"]) & 0xFFFFFFFF == (mbh * NPIC if aq else 0)
    finally:
        e.close(); oe.close()


# ---------------------------------------------------------------- direction
def _psnr(a, b, mask):
    d = (a.astype(np.int64) - b.astype(np.int64))[mask]
    return 10 * np.log10(255.0 ** 2 * d.size / max(int((d * d).sum()), 1))


def test_the_bits_move_towards_the_rectangle(E):
    """fixed QP 34, 640 x 368, a -8 rectangle with feather 2 and balance 6: luma PSNR inside the rectangle is strictly higher than without a map, luma PSNR
    outside the feather is not higher.  Direction, not size: no thresholds"""
    w, h = 640, 368
    clip = _clip(w, h)
    cfg = dict(rects=[(208, 112, 224, 144, -8, 2)], balance=6)
    t, active, bg = R.roi_map(cfg, None, w // 16, h // 16)
    assert active and bg > 0
    inside = np.repeat(np.repeat(t == -8, 16, 0), 16, 1)
    outside = np.repeat(np.repeat(t == bg, 16, 0), 16, 1)
    assert inside.any() and outside.any()
    psnr = {}
    for on in (False, True):
        e = E.Encoder(w, h, gop=GOP, fixed_qp=34, exclusive=True)
        try:
            if on:
                e.set_roi(cfg)
            acc = []
            for i, (yp, _, y, uv) in enumerate(clip[:5]):
                e.encode(y, uv, pts=i)
                ry = e.fetch(E.FETCH_RECON_Y)
                acc.append((_psnr(ry, yp, inside), _psnr(ry, yp, outside)))
            psnr[on] = np.mean(acc, axis=0)
            assert e.last_roi() == ((True, bg, int(t.astype(np.int64).sum())) if on else (False, 0, 0))
        finally:
            e.close()
    assert psnr[True][0] > psnr[False][0], psnr
    assert psnr[True][1] <= psnr[False][1], psnr
