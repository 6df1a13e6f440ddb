"""Periodic intra refresh, CPU side: the schedule of tests/irref.py, and its clean bounds pinned to the standard through the independent decoder.

Hand-built P pictures go through the product's slice writer on top of an IDR picture the oracle encoded from noise.  Each is decoded twice, once
with the true reference and once with the reference corrupted right of the clean bound (the decoder's reference planes are overwritten between the
IDR picture and the P picture), and the two decodes are compared."""
import json
import os
import subprocess

import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import irref
from tests.test_boundary_cpu import PROBE, gst_env, needs_gst

W, H = 176, 144
MBW, MBH = W // 16, H // 16
QP = 45  # alpha 144 / beta 15: the filter is active across the edges of the noise picture below, and strong across an intra edge


# ---- the schedule
@pytest.mark.parametrize("mbw,n", [(120, 60), (80, 60), (11, 60), (11, 7), (240, 30), (8, 2), (5, 8)])
def test_every_column_is_refreshed_within_a_cycle(mbw, n):
    pics = irref.schedule(mbw, n, ["idr"] + ["p"] * (3 * n))
    for c in range(3):
        cyc = pics[1 + c * n:1 + (c + 1) * n]
        assert [p["j"] for p in cyc] == list(range(n)) and cyc[0]["start"] and not any(p["start"] for p in cyc[1:])
        hit = np.zeros(mbw, int)
        for p in cyc:
            assert p["c0"] == max(irref.a_col(p["j"], mbw, n) - 1, 0) and p["c1"] == irref.a_col(p["j"] + 1, mbw, n)
            hit[p["c0"]:p["c1"]] += 1
        assert (hit >= 1).all()                                  # every column within N pictures
        assert cyc[-1]["c1"] == mbw and irref.exact_cols(cyc[-1], mbw) == (16 * mbw, 8 * mbw)
        # the overlap: every column but the cycle's last is refreshed again by the next picture that moves on
        assert all(b["c0"] <= max(a["c1"] - 1, 0) for a, b in zip(cyc, cyc[1:]))


def test_cycles_restart_after_an_idr_picture():
    mbw, n = 20, 6
    wants = ["idr"] + ["p"] * 8 + ["idr"] + ["p"] * 7
    pics = irref.schedule(mbw, n, wants)
    assert [p["j"] for p in pics] == [-1, 0, 1, 2, 3, 4, 5, 0, 1, -1, 0, 1, 2, 3, 4, 5, 0]
    assert [i for i, p in enumerate(pics) if p["start"]] == [1, 7, 10, 16]
    assert pics[10]["c0"] == 0 and pics[10]["clean"] == -1     # nothing is clean right after the cycle restarts


def test_all_skip_pictures_carry_the_refresh_over():
    mbw, n = 20, 5
    pics = irref.schedule(mbw, n, ["idr", "p", "skip", "p", "p", "skip", "p", "p"])
    # j:                             -1    0    1      2    3    4(last: not skipped) 0(skipped instead) 1
    assert [p["kind"] for p in pics] == ["idr", "p", "skip", "p", "p", "p", "skip", "p"]
    assert pics[2]["R"] == 4 and pics[3]["c0"] == 3 and pics[3]["c1"] == 12 and pics[3]["clean"] == 16 * 4 - 4   # from max(R - 1, 0) on
    assert pics[5]["j"] == 4 and pics[5]["c1"] == mbw
    assert pics[6]["start"] and pics[7]["c0"] == 0 and pics[7]["c1"] == 8   # the skipped cycle start refreshed nothing


def test_clean_bounds_and_the_intra_4x4_restriction():
    mbw, n = 12, 4
    pic = irref.schedule(mbw, n, ["idr", "p", "p"])[2]         # j = 1: columns [2, 6), clean luma <= 44
    assert (pic["c0"], pic["c1"], pic["clean"]) == (2, 6, 44)
    assert all(irref.vector_ok(0, v, pic) for v in range(-67, 68))   # column 0 (c0 - 2) is far enough from the bound for any vector of +-16.75
    assert irref.vector_ok(1, 4 * 13, pic) and not irref.vector_ok(1, 4 * 13 + 1, pic)   # 31 + 13 = 44; a fraction adds 3
    assert irref.vector_ok(1, 4 * 10 + 3, pic) and not irref.vector_ok(1, 4 * 11 + 1, pic)
    assert irref.vector_ok(2, 64, pic) and irref.vector_ok(9, 64, pic)   # refresh and dirty columns are not bound
    assert not irref.i4_mode_ok(pic, 5, mbw, 5, 3) and not irref.i4_mode_ok(pic, 5, mbw, 5, 7)
    assert irref.i4_mode_ok(pic, 5, mbw, 4, 3) and irref.i4_mode_ok(pic, 4, mbw, 5, 3) and irref.i4_mode_ok(pic, 5, mbw, 5, 8)
    last = irref.schedule(mbw, n, ["idr"] + ["p"] * n)[n]
    assert last["c1"] == mbw and irref.i4_mode_ok(last, mbw - 1, mbw, 5, 3)   # nothing unrefreshed above-right of the last column
    # luma is the binding bound for a 16x16 partition: every luma-legal vector is chroma-legal
    for clean in range(12, 16 * mbw, 16):
        for mx in range(mbw):
            for v in range(-70, 70):
                if irref.luma_ok(mx, v, clean):
                    assert irref.chroma_ok(mx, v, clean), (clean, mx, v)


# ---- the bounds against the independent decoder
@pytest.fixture(scope="module")
def idr(oracle):
    g = np.random.default_rng(0x1DE)
    y = g.integers(102, 110, (H, W), dtype=np.uint8)                # low-amplitude noise: neighbouring samples stay within beta
    uv = g.integers(124, 132, (H // 2, W), dtype=np.uint8)
    oe = oracle.Encoder(W, H, gop=30, threads=1)
    au, key = oe.encode(y, uv, QP)
    oe.close()
    assert key
    return au


def _records(kinds, mvx=None):
    """kinds[mx]: 'i' an Intra_16x16 DC macroblock, 'p' an inter macroblock (vector mvx[mx], 0); no residual anywhere"""
    mbi = np.zeros(MBW * MBH, E.MBINFO_DTYPE)
    for n in range(MBW * MBH):
        mx = n % MBW
        mbi[n]["qp"] = QP
        if kinds[mx] == "i":
            mbi[n]["mb_type"], mbi[n]["i16_mode"], mbi[n]["chroma_mode"] = 0, 2, 0
        else:
            mbi[n]["mb_type"], mbi[n]["mvx"] = 1, (mvx[mx] if mvx else 0)
    return mbi, np.zeros((MBW * MBH, E.LEVELS_PER_MB), np.int16)


def _decode(oracle, idr_au, p_au, dirty_y=None, dirty_uv=None, by=100):
    """decode the IDR picture, corrupt the reference's luma columns >= dirty_y and chroma columns >= dirty_uv (+by), decode the P picture"""
    dec = oracle.Decoder()
    assert dec.decode(idr_au) is not None
    ry = oracle._view(dec.L.orc_dec_y(dec.h), (16 * MBH, 16 * MBW), np.uint8)
    ruv = oracle._view(dec.L.orc_dec_uv(dec.h), (8 * MBH, 16 * MBW), np.uint8)
    if dirty_y is not None:
        ry[:, dirty_y:] = np.clip(ry[:, dirty_y:].astype(int) + by, 0, 255)
    if dirty_uv is not None:
        ruv[:, 2 * dirty_uv:] = np.clip(ruv[:, 2 * dirty_uv:].astype(int) + by, 0, 255)
    y, uv = dec.decode(p_au)
    dec.close()
    return y, uv


def _first_diff_col(a, b, step=1):
    d = np.nonzero((a != b).any(axis=0))[0]
    return int(d[0]) // step if d.size else None


def _p_au(mbi, lev):
    E.host_set_p_slices(0, 0)
    return E.host_write_headers(W, H, 60) + E.host_write_slice(MBW, MBH, False, 1, 0, QP, mbi, lev)


@pytest.mark.parametrize("a", [1, 3, 6, 10])
def test_deblocking_dirt_reaches_exactly_the_last_three_luma_and_last_chroma_column(oracle, idr, a):
    """(a) Refresh columns [0, a) intra, the rest copies a reference that is corrupted right of the clean bound 16 a - 4 / 8 a - 2: the decoded
    picture is exact up to luma column 16 a - 4 and chroma column 8 a - 2, and not beyond -- the filter of the edge at 16 a reaches three luma
    samples and one chroma sample into the refreshed side."""
    mbi, lev = _records(["i"] * a + ["p"] * (MBW - a))
    au = _p_au(mbi, lev)
    y0, uv0 = _decode(oracle, idr, au)
    y1, uv1 = _decode(oracle, idr, au, 16 * a - 3, 8 * a - 1, by=24)  # (|p0 - q0| stays below (alpha >> 2) + 2: the strong filter runs in both decodes)
    assert _first_diff_col(y0, y1) == 16 * a - 3
    u0, u1 = uv0.reshape(8 * MBH, -1, 2), uv1.reshape(8 * MBH, -1, 2)
    assert min(_first_diff_col(u0[..., c], u1[..., c]) for c in (0, 1)) == 8 * a - 1


@pytest.mark.parametrize("R", [2, 4, 9])
def test_vectors_at_the_clean_bound_decode_identically_and_one_quarter_past_do_not(oracle, idr, R):
    """(b), (c) Column R - 2 (the only one a vector of <= 16.75 samples can take past the bound) inter with the vector under test, the other
    columns left of R - 1 inter with the zero vector, columns [R - 1, mbw) refresh columns.  With the reference corrupted right of the clean bound
    the picture decodes identically for every vector irref accepts and differently for the next quarter sample -- luma and chroma separately."""
    mx = R - 2
    pic = dict(kind="p", c0=R - 1, c1=MBW, clean=16 * R - 4)
    cands = range(-64, 68)
    luma_legal = [v for v in cands if irref.luma_ok(mx, v, pic["clean"])]
    chroma_legal = [v for v in cands if irref.chroma_ok(mx, v, pic["clean"])]
    vl, vc = max(v for v in luma_legal if v % 4 == 0), max(chroma_legal)
    assert vl + 1 not in luma_legal and vc + 1 not in chroma_legal
    assert max(v for v in luma_legal if v % 4) == vl - 9          # the last fractional one reads the bound column through its sixth tap

    def run(v, dirty_y, dirty_uv):
        mvx = [0] * MBW
        mvx[mx] = v
        mbi, lev = _records(["p"] * (R - 1) + ["i"] * (MBW - R + 1), mvx)
        au = _p_au(mbi, lev)
        return _decode(oracle, idr, au), _decode(oracle, idr, au, dirty_y, dirty_uv)

    for v in (vl, vl - 8, vl - 9, vl - 10, vl - 11):               # luma: the bound, and the whole and fractional vectors below it
        (y0, _), (y1, _) = run(v, 16 * R - 3, None)
        assert np.array_equal(y0, y1), v
    for v in (vl + 1, vl + 2, vl + 3, vl - 7):                      # one quarter sample past a whole-sample vector at the bound (vl - 8 is one)
        (y0, _), (y1, _) = run(v, 16 * R - 3, None)
        assert not np.array_equal(y0, y1), v
    (_, c0), (_, c1) = run(vc, None, 8 * R - 1)
    assert np.array_equal(c0, c1)
    (_, c0), (_, c1) = run(vc + 1, None, 8 * R - 1)
    assert not np.array_equal(c0, c1)


# ---- the element
@needs_gst
@pytest.mark.skipif(not os.path.exists(PROBE), reason="probe not built")
@pytest.mark.parametrize("line,want", [("mi355h264enc", 0), ("mi355h264enc intra-refresh=true key-int-max=30", 1), ("mi355h264enc speed-preset=2 intra-refresh=1", 1)])
def test_element_intra_refresh_property(line, want):
    """x264enc's `intra-refresh` boolean, default false, read back through GObject (no device involved)."""
    r = subprocess.run([PROBE, "videotestsrc ! %s name=venc_kbps ! appsink name=appsink" % line, "--props"], env=gst_env(), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.splitlines()[-1])["intra_refresh"] == want


def test_intra_refresh_setter_is_exported():
    assert "mi355enc_set_intra_refresh" in E.EXPORTS
    assert hasattr(E.load(), "mi355enc_set_intra_refresh")
