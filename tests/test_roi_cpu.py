"""Region-of-interest quantisation, host side (no device): mi355enc_roi_map against the numpy rule of tests/roiref.py on hand-picked
cases and on seeded random configurations at six picture sizes, every refusal, the element's string form, the ABI's version and export names, and the oracle
composed under a map -- an IDR picture and a P picture behind it through the oracle's stage functions with orc_set_aq_map, which must decode in the oracle's
own decoder to the composed reconstruction with QP_Y = clamp(qp + t) wherever a delta is sent and every delta inside -26 .. +25.  The GPU tests
(tests/test_roi_gpu.py) hold the device against the same composed pictures."""
import ctypes as C

import numpy as np
import pytest

from tests import roiref as R


def _both(E, cfg, user, mbw, mbh):
    got, want = E.roi_map(cfg, user, mbw, mbh), R.roi_map(cfg, user, mbw, mbh)
    assert got[0].dtype == np.int8 and got[0].shape == (mbh, mbw)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (cfg, mbw, mbh, got[1:], want[1:])
    return got


def test_map_by_hand(E):
    """the rule on cases small enough to write down"""
    # one rectangle covering macroblock (1, 1) of 5 x 3, delta -6, feather 2: ring 1 is -(6 * 2 // 3) = -4, ring 2 -(6 * 1 // 3) = -2
    t, active, bg = _both(E, dict(rects=[(16, 16, 16, 16, -6, 2)], balance=0), None, 5, 3)
    assert t.tolist() == [[-4, -4, -4, -2, 0], [-4, -6, -4, -2, 0], [-4, -4, -4, -2, 0]] and active and bg == 0
    # a rectangle of one sample at a macroblock's last sample, and one that crosses into the next macroblock by one sample
    assert _both(E, dict(rects=[(31, 15, 1, 1, 3, 0)]), None, 5, 3)[0].tolist() == [[0, 3, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert _both(E, dict(rects=[(31, 15, 2, 2, 3, 0)]), None, 5, 3)[0].tolist() == [[0, 3, 3, 0, 0], [0, 3, 3, 0, 0], [0, 0, 0, 0, 0]]
    # emphasis wins over a positive rectangle that covers it; outside the emphasis the positive one stays
    t = _both(E, dict(rects=[(0, 0, 80, 48, 5, 0), (32, 16, 16, 16, -3, 1)]), None, 5, 3)[0]
    assert t.tolist() == [[5, -1, -1, -1, 5], [5, -1, -3, -1, 5], [5, -1, -1, -1, 5]]
    # balance, uncapped: S = -6 - 8 * 4 - 3 * 2 = -44 over N0 = 3 zeros -> (44 + 1) // 3 = 15 -> the cap 12; with cap 0 nothing
    t, active, bg = _both(E, dict(rects=[(16, 16, 16, 16, -6, 2)], balance=12), None, 5, 3)
    assert bg == 12 and t[:, 4].tolist() == [12, 12, 12]
    t, active, bg = _both(E, dict(rects=[(16, 16, 16, 16, -1, 0)], balance=12), None, 5, 3)
    assert bg == 0 and active and t.sum() == -1  # (1 + 7) // 14 = 0: nothing to spread
    t, active, bg = _both(E, dict(rects=[(16, 16, 16, 16, -12, 0)], balance=5), None, 5, 3)
    assert bg == 1 and t.sum() == -12 + 14  # (12 + 7) // 14 = 1, under the cap
    # balance with no zero left (N0 = 0), and with S >= 0
    assert _both(E, dict(rects=[(0, 0, 80, 48, -2, 0)], balance=6), None, 5, 3)[1:] == (True, 0)
    assert _both(E, dict(rects=[(0, 0, 16, 16, 4, 0), (64, 32, 16, 16, -4, 0)], balance=6), None, 5, 3)[1:] == (True, 0)
    # a rectangle wholly outside: nothing, feather included, no error; inactive
    for r in [(80, 0, 16, 16, -6, 8), (-16, 0, 16, 16, -6, 8), (0, 48, 16, 16, -6, 8), (0, -16, 16, 16, -6, 8), (-65536, -65536, 65536, 65536, 5, 8)]:
        t, active, bg = _both(E, dict(rects=[r], balance=6), None, 5, 3)
        assert not t.any() and not active and bg == 0
    # the caller's map alone, with and without a configuration; clamped against a rectangle
    user = np.arange(-7, 8, dtype=np.int8).reshape(3, 5)
    assert np.array_equal(_both(E, None, user, 5, 3)[0], user)
    assert np.array_equal(_both(E, dict(rects=[], balance=0), user, 5, 3)[0], user)
    assert _both(E, dict(rects=[(0, 0, 80, 48, -12, 0)]), user, 5, 3)[0].min() == -12
    assert _both(E, None, np.zeros((3, 5), np.int8), 5, 3)[1:] == (False, 0) and _both(E, None, None, 5, 3)[1:] == (False, 0)


@pytest.mark.parametrize("edge", ["left", "right", "top", "bottom"])
def test_feather_reaching_past_each_picture_edge(E, edge):
    """the ramp is cut at the picture's edge, never wrapped or shifted"""
    mbw, mbh = 21, 12
    x, y = {"left": (16, 80), "right": (16 * 19, 80), "top": (160, 16), "bottom": (160, 16 * 10)}[edge]
    t = _both(E, dict(rects=[(x, y, 16, 16, -9, 8)], balance=0), None, mbw, mbh)[0]
    assert t[y // 16, x // 16] == -9 and t.min() == -9 and (t <= 0).all()
    assert (t[:, 0] if edge == "left" else t[:, -1] if edge == "right" else t[0] if edge == "top" else t[-1]).min() == -(9 * 8 // 9)  # one macroblock from the rectangle


def test_map_random_configurations(E):
    """200 seeded configurations spread over the six sizes, every other one with a caller's map"""
    g = R.Rng(0xC0FFEE)
    sizes = [(1, 1), (4, 3), (5, 3), (21, 12), (45, 25), (512, 512)]
    seen_bg = seen_clamp = 0
    for i in range(200):
        mbw, mbh = sizes[i % 6]
        cfg = R.random_cfg(g, mbw, mbh)
        user = np.random.default_rng(i).integers(-12, 13, (mbh, mbw)).astype(np.int8) if i & 1 else None
        t, active, bg = _both(E, cfg, user, mbw, mbh)
        seen_bg += bg > 0
        seen_clamp += int(abs(t).max()) == 12
    assert seen_bg > 10 and seen_clamp > 10


FIELD_RANGES = [("n_rects", 0, 8), ("x", -65536, 65536), ("y", -65536, 65536), ("w", 1, 65536), ("h", 1, 65536), ("delta", -12, 12), ("feather", 0, 8), ("balance", 0, 12)]


@pytest.mark.parametrize("name,lo,hi", FIELD_RANGES)
def test_refusals_one_step_outside(E, name, lo, hi):
    for v, ok in ((lo - 1, False), (lo, True), (hi, True), (hi + 1, False)):
        cfg = R.with_field(name, v)
        if name == "n_rects" and v > 8:  # (the mirror's roi() refuses nine rectangles itself: through the structure)
            c = E.roi(R.with_field(name, 8))
            c.n_rects = v
        elif name == "n_rects" and v < 0:
            c = E.roi(R.BASE)
            c.n_rects = v
        else:
            c = E.roi(cfg)
        assert (E.roi_check(c) == 0) == ok, (name, v)
        if not ok:
            out = np.full(15, 77, np.int8)
            assert E.load().mi355enc_roi_map(C.byref(c), None, 5, 3, out.ctypes.data_as(C.c_void_p), None, None) == E.ERR_ARG and (out == 77).all()
    assert E.roi_check(E.roi([(0, 0, 16, 16, 0, 0)])) == E.ERR_ARG  # delta 0 says nothing
    assert E.load().mi355enc_roi_check(None) == E.ERR_ARG


def test_refusals_of_the_callers_map_and_the_size(E):
    L = E.load()
    for bad in (-13, 13, -128, 127):
        for at in (0, 7, 14):
            user = np.zeros(15, np.int8)
            user[at] = bad
            out = np.full(15, 77, np.int8)
            assert L.mi355enc_roi_map(None, user.ctypes.data_as(C.c_void_p), 5, 3, out.ctypes.data_as(C.c_void_p), None, None) == E.ERR_ARG and (out == 77).all()
            with pytest.raises(E.EncoderError):
                E.roi_map(None, user, 5, 3)
    out = np.zeros(4, np.int8)
    for mbw, mbh in ((0, 1), (1, 0), (513, 1), (1, 513), (-1, -1)):
        assert L.mi355enc_roi_map(None, None, mbw, mbh, out.ctypes.data_as(C.c_void_p), None, None) == E.ERR_ARG
    assert L.mi355enc_roi_map(None, None, 1, 1, None, None, None) == E.ERR_ARG


def _text(cfg):
    return ";".join(",".join(str(v) for v in r) for r in cfg["rects"])


def test_parse_round_trips_what_it_accepts(E):
    g = R.Rng(0xBEEF)
    for i in range(100):
        cfg = R.random_cfg(g, 45, 25)
        c = E.roi_parse(_text(cfg), balance=cfg["balance"])
        assert c.as_dict() == dict(rects=[tuple(r) for r in cfg["rects"]], balance=cfg["balance"]), i
        assert _text(c.as_dict()) == _text(cfg)
    assert E.roi_parse("").as_dict() == dict(rects=[], balance=0) and E.roi_parse(" \t", 4).as_dict() == dict(rects=[], balance=4)
    assert E.roi_parse("16,32,640,360,-6").as_dict()["rects"] == [(16, 32, 640, 360, -6, 0)]  # the feather is optional
    assert E.roi_parse(" 1 , 2 ,3,4, +5 , 6 ;-7,-8,9,10,-11").as_dict()["rects"] == [(1, 2, 3, 4, 5, 6), (-7, -8, 9, 10, -11, 0)]


JUNK = ["x", "1,2,3,4", "1,2,3,4,0", "1,2,3,4,13", "1,2,3,4,-13", "1,2,3,4,5,9", "1,2,3,4,5,-1", "1,2,3,4,5,6,7", "1,2,3,4,5;", ";1,2,3,4,5", "1,2,3,4,5;;1,2,3,4,5", "1,,3,4,5",
        "1,2,0,4,5", "1,2,3,65537,5", "65537,2,3,4,5", "1 2,3,4,5,6", "1,2,3,4,5x", "99999999999999999999,2,3,4,5", "1,2,3,4,-", "1.5,2,3,4,5", "0x10,2,3,4,5", "1,2,3,4,5\n",
        ";".join(["1,1,1,1,1"] * 9)]


@pytest.mark.parametrize("text", JUNK)
def test_parse_refuses_junk_without_touching_the_output(E, text):
    c = E.roi([(9, 8, 7, 6, 5, 4)], balance=3)
    before = bytes(c)
    assert E.load().mi355enc_roi_parse(text.encode(), C.byref(c)) == E.ERR_ARG and bytes(c) == before
    with pytest.raises(E.EncoderError):
        E.roi_parse(text)


def test_abi_version_and_export_names(E):
    L = E.load()
    assert L.mi355enc_abi_version() == 4
    new = [n for n in E.EXPORTS if "roi" in n]
    assert len(new) == 10 and not any(n.startswith("mi355enc_stage_") for n in new)
    for n in new:
        getattr(L, n)
    assert C.sizeof(E.Roi) == 4 * (1 + 6 * 8 + 1)
    c = E.Roi()
    c.n_rects = 5
    L.mi355enc_roi_default(C.byref(c))
    assert c.as_dict() == dict(rects=[], balance=0)
    # the handle entry points refuse a null handle before anything else
    assert L.mi355enc_set_roi(None, None, None) == E.ERR_ARG and L.mi355enc_get_roi(None, None, None) == E.ERR_ARG and L.mi355enc_last_roi(None, None, None, None) == E.ERR_ARG
    assert L.mi355enc_debug_roi_bytes(None) == 0 and L.mi355enc_roi_probe_set_map(None, None) == E.ERR_ARG and L.mi355enc_roi_probe_offsets(None, None, None) == E.ERR_ARG


@pytest.mark.parametrize("qp", R.QPS_COMPOSED)
@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("w,h", R.SIZES_COMPOSED)
def test_the_oracle_composed_under_a_map(oracle, w, h, slices, qp):
    """IDR + P under the test map: compose_idr / compose_p assert the decode, QP_Y and the delta range themselves; here: the map did something, deltas were
    sent in both pictures, both clamps of QP_Y are reached where the QP allows, and without the map the composition is the oracle encoder's own stream"""
    c = R.composed(w, h, slices, qp)
    t = c["t"]
    assert t.min() == -12 and t.max() == 12
    for pic in (c["idr"], c["p"]):
        assert pic["deltas"].size > 0 and np.abs(pic["deltas"]).max() > 0, "no mb_qp_delta other than 0 was sent"
    sent = R.sends_delta(c["idr"]["mbi"])
    q = c["idr"]["mbi"]["qp"][sent]
    assert (qp != 6 or q.min() == 0) and (qp != 45 or q.max() == 51) and len(np.unique(q)) > 2
    if qp == 30:  # the composition itself: with a map of zeros it is what oracle.Encoder writes
        dec = oracle.Decoder()
        z = np.zeros_like(t)
        (y0, uv0, vy0, vuv0), (y1, uv1, vy1, vuv1) = c["clip"]
        idr = R.compose_idr(oracle, dec, w, h, y0, uv0, qp, z, c["rows"], c["dbf"])
        p = R.compose_p(oracle, dec, w, h, y1, uv1, y0, idr["rec_y"], idr["rec_uv"], qp, z, c["rows"], c["dbf"])
        oe = oracle.Encoder(w, h, gop=30, threads=8, intra_slices=slices, p_slices=slices, slice_deblock_local=slices > 1)
        assert oe.encode(vy0, vuv0, qp)[0] == idr["au"] and oe.encode(vy1, vuv1, qp)[0] == p["au"]
        assert np.array_equal(oe.recon_y, p["rec_y"])
        oe.close()
        dec.close()
