"""The per-macroblock transform size choice (cfg.transform8x8 = 2), CPU side: the test reference in tests/t8ref.py (luma prediction, the SA8D / SATD rule)
against the oracle and against residuals worked by hand, and pictures that mix 4x4 and 8x8 inter macroblocks through the product's slice writer, the
oracle's writer, the oracle's deblocker and the independent decoder."""
import json
import os
import subprocess

import numpy as np
import pytest

from ceracoder_amd import enc as E
from ceracoder_amd import synth
from tests import t8ref
from tests.test_boundary_cpu import PROBE, gst_env, needs_gst
from tests.util import frames, pad_planes

NZ_T8 = 1 << 27


def _clip(kind, w, h, n):
    if kind == "s2":
        return [f[:2] for f in frames(w, h, n)]
    gen = synth.s4_frames(w, h, n, pan_after=0) if kind == "s4pan" else synth.s4_frames(w, h, n)
    return [pad_planes(y, uv) for y, uv in gen]


def _field(oracle, cy, ry, qp, iters=3):
    surf, imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
    for _ in range(iters):
        imv = oracle.me_select(surf, imv, cy.shape[1] // 16, cy.shape[0] // 16, 16, qp, threads=8)
    return surf, imv


# ---- the prediction: every inter macroblock without luma levels reconstructs as its prediction
@pytest.mark.parametrize("kind,w,h", [("s2", 176, 144), ("s2", 320, 192), ("s4pan", 320, 192), ("s4", 640, 368)])
@pytest.mark.parametrize("drop", [12, 6])
def test_prediction_equals_the_oracles(oracle, kind, w, h, drop):
    """oracle.pmb_frame on the rate control's drop ladder: the macroblocks it codes as prediction only (the skip probe, the ladder, or nothing left after
    quantisation) have recon == prediction at their record's vector; t8ref.luma_pred must give exactly that, vectors leaving the picture included."""
    (cy, cuv), (ry, ruv) = _clip(kind, w, h, 2)[1], _clip(kind, w, h, 2)[0]
    qp = 30
    surf, imv = _field(oracle, cy, ry, qp)
    rec_y, _, mbi, _, _ = oracle.pmb_frame(cy, cuv, ry, ruv, imv, surf, qp, drop=drop, threads=8)
    mbh, mbw = cy.shape[0] // 16, cy.shape[1] // 16
    H, W = cy.shape
    checked = outside = frac = 0
    for n in range(mbw * mbh):
        m = mbi[n]
        if m["mb_type"] != 1 or (int(m["nzmask"]) & 0xFFFF) or m["i16_mode"]:
            continue
        mby, mbx = divmod(n, mbw)
        mvx, mvy = int(m["mvx"]), int(m["mvy"])
        pred = t8ref.luma_pred(ry, 16 * mbx, 16 * mby, mvx, mvy)
        assert np.array_equal(pred, rec_y[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16]), (n, mvx, mvy)
        checked += 1
        X, Y = 16 * mbx + (mvx >> 2), 16 * mby + (mvy >> 2)
        outside += X - 2 < 0 or Y - 2 < 0 or X + 19 > W or Y + 19 > H
        frac += (mvx & 3) != 0 or (mvy & 3) != 0
    assert checked > mbw * mbh // 4 and outside > 0  # vectors whose filter window leaves the picture (clamped reference samples)
    if drop < 12:
        assert frac > 0  # refined vectors (at drop 12 every macroblock is P_Skip at its whole-sample predictor)


def test_prediction_covers_every_quarter_sample_position():
    """All sixteen fractional positions against a direct evaluation of 8.4.2.2.1's equations for one sample."""
    g = np.random.Generator(np.random.PCG64(7))
    ref = g.integers(0, 256, (48, 48)).astype(np.uint8)
    R = ref.astype(np.int64)

    def tap(v):
        return v[0] - 5 * v[1] + 20 * v[2] + 20 * v[3] - 5 * v[4] + v[5]

    def c1(v):
        return min(255, max(0, v))

    x, y = 20, 17  # the sample (4, 1) of the macroblock at (16, 16) with whole-sample vector 0
    b1 = lambda yy: tap([R[yy, x - 2 + k] for k in range(6)])
    h1 = lambda xx: tap([R[y - 2 + k, xx] for k in range(6)])
    b, h, s, m = c1((b1(y) + 16) >> 5), c1((h1(x) + 16) >> 5), c1((b1(y + 1) + 16) >> 5), c1((h1(x + 1) + 16) >> 5)
    j = c1((tap([b1(y - 2 + k) for k in range(6)]) + 512) >> 10)
    G, Hs, M = R[y, x], R[y, x + 1], R[y + 1, x]
    a = lambda p, q: (p + q + 1) >> 1
    want = {(0, 0): G, (1, 0): a(G, b), (2, 0): b, (3, 0): a(Hs, b), (0, 1): a(G, h), (1, 1): a(b, h), (2, 1): a(b, j), (3, 1): a(b, m),
            (0, 2): h, (1, 2): a(h, j), (2, 2): j, (3, 2): a(j, m), (0, 3): a(M, h), (1, 3): a(h, s), (2, 3): a(j, s), (3, 3): a(m, s)}
    for (xf, yf), v in want.items():
        assert t8ref.luma_pred(ref, 16, 16, xf, yf)[1, 4] == v, (xf, yf)


# ---- the rule on residuals worked by hand
def test_zero_residual_keeps_4x4():
    d = np.zeros((16, 16), np.int64)
    assert t8ref.raw4(d) == 0 and t8ref.raw8(d) == 0
    assert not t8ref.decide_residual(d)  # 0 < 0 is false: a tie goes to 4x4


def test_constant_8x8_block_takes_8x8():
    """c over one 8x8 block: four 4x4 DCs of 16 c (raw4 = 64 c), one 8x8 DC of 64 c (raw8 = 64 c); (64 c + 2) >> 2 = 16 c < 32 c."""
    d = np.zeros((16, 16), np.int64)
    d[8:16, 0:8] = 5
    assert t8ref.raw4(d) == 320 and t8ref.raw8(d) == 320
    assert t8ref.decide_residual(d)


@pytest.mark.parametrize("i,j", [(0, 0), (1, 2), (3, 3)])
def test_hadamard_basis_pattern_in_one_4x4_block_keeps_4x4(i, j):
    """c h_i h_j^T in one 4x4 block: one coefficient of 16 c (raw4 = 16 c); in its 8x8 block the pattern sits in one quadrant, which H8 = [[H4, H4],
    [H4, -H4]] spreads over all four quadrants (raw8 = 64 c); (64 c + 2) >> 2 = 16 c is not below 8 c."""
    c = 3
    d = np.zeros((16, 16), np.int64)
    d[4:8, 8:12] = c * np.outer(t8ref.H4[i], t8ref.H4[j])
    assert t8ref.raw4(d) == 16 * c and t8ref.raw8(d) == 64 * c
    assert not t8ref.decide_residual(d)


def test_worked_example_horizontal_ramp():
    """D[y, x] = x.  A 4x4 block starting at column a: H4 r = (4a + 6, -2, -4, 0) for r = (a .. a + 3) and the rows are equal, so its sum is 4 (4a + 12):
    48, 112, 176, 240 along a row of blocks, raw4 = 4 x 576 = 2304.  An 8x8 block at column a: H8 r = (8a + 28, -4, -8, 0, -16, 0, 0, 0), sum 8 (8a + 56):
    448 and 960, raw8 = 2 x 1408 = 2816.  (2816 + 2) >> 2 = 704 < 2304 >> 1 = 1152: 8x8."""
    d = np.tile(np.arange(16, dtype=np.int64), (16, 1))
    assert t8ref.raw4(d) == 2304
    assert t8ref.raw8(d) == 2816
    assert t8ref.decide_residual(d)


def test_raw4_is_the_oracles_satd(oracle):
    """orc_satd16 (the refinement's measure) is raw4 halved"""
    g = np.random.Generator(np.random.PCG64(11))
    for _ in range(20):
        src, pred = g.integers(0, 256, (16, 16)).astype(np.uint8), g.integers(0, 256, (16, 16)).astype(np.uint8)
        assert t8ref.raw4(src.astype(np.int64) - pred) >> 1 == oracle.satd16(src, pred)


def test_raw8_is_invariant_to_the_hadamard_row_order():
    """The rule names no row order of H8 (a sum of magnitudes): the sequency-ordered matrix gives the same raw8."""
    g = np.random.Generator(np.random.PCG64(5))
    d = g.integers(-255, 256, (16, 16)).astype(np.int64)
    seq = t8ref.H8[np.argsort([(np.diff(r) != 0).sum() for r in t8ref.H8])]
    want = sum(int(np.abs(seq @ d[y:y + 8, x:x + 8] @ seq.T).sum()) for y in (0, 8) for x in (0, 8))
    assert t8ref.raw8(d) == want


# ---- pictures that mix the two transforms through the writers, the deblocker and the decoder
def _intra_p_pass(oracle, cy, cuv, rec_y, rec_uv, qp, idec, mbi, lev):
    H, W = cy.shape
    oracle.lib().orc_intra_p_frame(oracle._ptr(cy), oracle._ptr(cuv), oracle._ptr(rec_y), oracle._ptr(rec_uv), W, W // 16, H // 16, qp,
                                   oracle._ptr(idec), oracle._ptr(mbi), oracle._ptr(lev))


def _sps_profile(au):
    i = au.find(b"\x00\x00\x01")
    while i >= 0:
        if au[i + 3] & 31 == 7:
            return au[i + 4]
        i = au.find(b"\x00\x00\x01", i + 3)
    return None


@pytest.mark.parametrize("kind,w,h,qp", [("s2", 176, 144, 26), ("s2", 320, 192, 34), ("s4pan", 640, 368, 30), ("s4", 320, 192, 22)])
@pytest.mark.parametrize("slices", [0, 3])
def test_spliced_pictures_write_and_decode(oracle, kind, w, h, qp, slices):
    """An IDR picture, then oracle.pmb_frame against its reconstruction with the 8x8 transform and without it: identical decisions before the intra
    pass; their inter macroblocks spliced in a fixed pattern (records, levels, reconstruction), then the intra macroblocks reconstructed on the spliced
    picture.  The product's writer (High profile) equals the oracle's byte for byte, and the independent decoder gives the oracle's deblocking of the
    spliced picture -- with one slice, and with slices and slice-local deblocking (disable_deblocking_filter_idc 2)."""
    clip = _clip(kind, w, h, 2)
    mbh, mbw = h // 16, w // 16
    runs = {}
    try:
        oracle.set_transform8x8(True)
        oe = oracle.Encoder(w, h, gop=30, threads=8)
        idr, key = oe.encode(clip[0][0], clip[0][1], qp)
        ry, ruv = oe.recon_y.copy(), oe.recon_uv.copy()
        oe.close()
        assert key and _sps_profile(idr) == 100
        hdr = E.host_write_headers(w, h, 60, transform8x8=2)
        assert hdr == oracle.write_headers(w, h, 60) and _sps_profile(hdr) == 100  # mode 2 sends mode 1's SPS / PPS
        (cy, cuv) = clip[1]
        rows = oracle.slice_rows_for(mbh, slices, True) if slices else 0
        surf, imv = _field(oracle, cy, ry, qp)
        oracle.set_slice_rows(rows)
        oracle.set_slice_deblock(2 if rows else 0)
        idec = oracle.intra_decide(oracle.intra_analyse(cy, cuv), mbw, mbh, qp, True)  # (intra availability stops at a slice's first row)
        for t8 in (False, True):
            oracle.set_transform8x8(t8)
            _, _, _, lev, (pre_mbi, pre_y, pre_uv) = oracle.pmb_frame(cy, cuv, ry, ruv, imv, surf, qp, idec=idec, threads=8)
            runs[t8] = (pre_mbi, lev, pre_y, pre_uv)
        oracle.set_transform8x8(True)
        m4, m8 = runs[False][0], runs[True][0]
        for f in ("mvx", "mvy", "mb_type", "i16_mode", "chroma_mode", "qp", "cost"):
            assert np.array_equal(m4[f], m8[f]), f
        inter = m4["mb_type"] == 1
        assert (~inter).sum() > 0 and inter.sum() > mbw * mbh // 2  # intra macroblocks in the P picture
        # splice: the inter macroblock n from the 8x8 run where (mbx + 2 mby) % 3 == 0
        mbi, lev = m4.copy(), runs[False][1].copy()
        rec_y, rec_uv = runs[False][2].copy(), runs[False][3].copy()
        take8 = np.zeros(mbw * mbh, bool)
        for n in range(mbw * mbh):
            mby, mbx = divmod(n, mbw)
            if not inter[n] or (mbx + 2 * mby) % 3:
                continue
            take8[n] = True
            mbi[n], lev[n] = m8[n], runs[True][1][n]
            rec_y[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16] = runs[True][2][16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16]
            rec_uv[8 * mby:8 * mby + 8, 16 * mbx:16 * mbx + 16] = runs[True][3][8 * mby:8 * mby + 8, 16 * mbx:16 * mbx + 16]
        t8_coded = (mbi["nzmask"] & NZ_T8) != 0
        assert t8_coded.any() and (inter & ~t8_coded & ((mbi["nzmask"] & 0xFFFF) != 0)).any()  # both kinds of coded inter macroblock
        assert not (t8_coded & ~take8).any()
        _intra_p_pass(oracle, cy, cuv, rec_y, rec_uv, qp, idec, mbi, lev)
        want = oracle.write_slice(mbw, mbh, False, 1, 0, qp, mbi, lev)
        E.host_set_p_slices(rows, 2 if rows else 0)
        assert E.host_write_slice(mbw, mbh, False, 1, 0, qp, mbi, lev, transform8x8=True) == want
        assert E.host_write_slice(mbw, mbh, False, 1, 0, qp, mbi, lev, transform8x8=2) == want  # any non-zero value is High
        db_y, db_uv = oracle.deblock_frame(rec_y, rec_uv, mbi)
        dec = oracle.Decoder()
        dy, duv = dec.decode(idr)
        assert np.array_equal(dy, ry) and np.array_equal(duv, ruv)
        dy, duv = dec.decode(want)
        assert np.array_equal(dy, db_y) and np.array_equal(duv, db_uv)
        dec.close()
    finally:
        oracle.set_transform8x8(False)
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)
        E.host_set_p_slices(0, 0)


# ---- the element's property, read back through GObject (no device)
@needs_gst
@pytest.mark.skipif(not os.path.exists(PROBE), reason="probe not built")
@pytest.mark.parametrize("line,want", [
    ("mi355h264enc", dict(dct8x8=0, dct8x8_adaptive=0)),
    ("mi355h264enc speed-preset=2 key-int-max=60", dict(speed_preset=2, dct8x8=1, dct8x8_adaptive=0)),  # speed-preset does not set it
    ("mi355h264enc dct8x8=true dct8x8-adaptive=true", dict(dct8x8=1, dct8x8_adaptive=1, i8x8=0)),
    ("mi355h264enc dct8x8-adaptive=true speed-preset=3", dict(speed_preset=3, dct8x8=1, dct8x8_adaptive=1, i8x8=1, aq_mode=1)),
    ("mi355h264enc dct8x8-adaptive=true", dict(dct8x8=0, dct8x8_adaptive=1)),  # (ignored without dct8x8: Constrained Baseline)
])
def test_dct8x8_adaptive_property_reads_back(line, want):
    r = subprocess.run([PROBE, "videotestsrc ! %s name=venc_kbps ! appsink name=appsink" % line, "--props"], env=gst_env(), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.splitlines()[-1])
    for k, v in want.items():
        assert got[k] == v, (k, got)
