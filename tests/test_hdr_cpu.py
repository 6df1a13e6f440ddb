"""HDR tone map without a device: the model's anchors against published numbers, the exported parameter block against one built in numpy
from the model, the integer rule against the double model over a sweep of the input cube, the rule's intermediates against the types section 22 names, and
mi355enc_hdr_tables' argument checks."""
import ctypes as C

import numpy as np
import pytest

from ceracoder_amd import enc as E
from tests import hdrref as H

# (transfer, full, peak, target, out_matrix, out_full): PQ at 1000 and 4000, HLG at 1000; target 100 and 203; matrices 1 and 6; both ranges on either side
SETS = [(H.PQ, 0, 1000, 203, 1, 0), (H.PQ, 0, 4000, 100, 6, 0), (H.PQ, 1, 1000, 100, 1, 1), (H.PQ, 0, 4000, 203, 6, 1),
        (H.HLG, 0, 1000, 203, 1, 0), (H.HLG, 1, 1000, 100, 6, 0), (H.HLG, 0, 1000, 100, 1, 1), (H.HLG, 1, 1000, 203, 6, 1)]
IDS = ["%s-%s-%d-%d-m%d-%s" % ("pq" if s[0] == H.PQ else "hlg", "full" if s[1] else "lim", s[2], s[3], s[4], "full" if s[5] else "lim") for s in SETS]


def sig3(x):
    return float("%.3g" % float(x))


# ---------------------------------------------------------------- the model against published numbers
# (These five check tests/hdrref.py's model alone, the yardstick everything else is held to: they call nothing of the library.)
def test_pq_anchors():
    assert sig3(H.pq_eotf(0.5081)) == 100.0
    assert sig3(H.pq_eotf(0.5807)) == 203.0
    assert sig3(H.pq_eotf(0.7518)) == 1000.0
    for l in (0.01, 1.0, 100.0, 4000.0, 10000.0):
        assert abs(float(H.pq_eotf(H.pq_inv(l))) / l - 1.0) < 1e-12


def test_hlg_reference_white():
    y, cb, cr = 64 + 0.75 * 876, 512, 512  # signal 0.75, grey
    r, g, b = H.model_light(H.HLG, 0, 1000, y, cb, cr)
    assert sig3(r) == sig3(g) == sig3(b) == 203.0


def test_tone_curve_anchors():
    assert np.array_equal(H.eetf(np.array([0.0, 1.0, 50.0, 87.0]), 1000, 203), [0.0, 1.0, 50.0, 87.0])  # below the knee: unchanged, exactly
    assert sig3(H.eetf(88.0, 1000, 203)) == 88.0 and float(H.eetf(89.0, 1000, 203)) < 88.995  # the knee: 88 cd/m^2
    assert sig3(H.eetf(203.0, 1000, 203)) == 159.0
    assert sig3(H.eetf(1000.0, 1000, 203)) == 203.0
    assert sig3(H.eetf(203.0, 1000, 100)) == 88.2
    n = np.linspace(0.0, 1000.0, 2001)
    assert np.all(np.diff(H.eetf(n, 1000, 203)) >= 0) and float(H.eetf(n, 1000, 203).max()) <= 203.0 + 1e-9
    assert np.array_equal(H.eetf(n[:800], 400, 400), n[:800])  # target >= peak: the identity


def test_gamut_matrix():
    m = np.array(H.gamut_matrix())
    assert np.allclose(m.sum(axis=1), 1.0, atol=1e-12)
    assert np.allclose(m[0], [1.6605, -0.5876, -0.0728], atol=5e-5)


def test_grey_at_18_nits():
    yy = H.pq_inv(18.0) * 876 + 64  # (not a code: the model takes any real)
    y8, cb, cr = H.model_out(1, 0, *H.model_rgb(H.PQ, 0, 1000, 203, yy, 512, 512))
    assert sig3(y8) == 75.2 and abs(float(cb) - 128) < 1e-9 and abs(float(cr) - 128) < 1e-9


# ---------------------------------------------------------------- the exported block against the one numpy builds from the model
@pytest.mark.parametrize("s", SETS, ids=IDS)
def test_exported_block_against_numpy(s):
    got, want = E.hdr_tables(*s).astype(np.int64), H.build_block(*s).astype(np.int64)
    assert got.shape == want.shape == (H.BLOCK_WORDS,)
    assert np.array_equal(got[:H.HDR_WORDS], want[:H.HDR_WORDS])  # header and matrices: + - * / and floor only, word for word
    assert got[3] == s[2] and got[4] == s[3] and got[7] == H.BLOCK_WORDS
    assert np.max(np.abs(got - want)) <= 1  # tables: libm's and numpy's pow / exp may differ in the last place
    lin, ga, gb, oe = (got[a:a + n] for a, n in ((H.LIN_AT, H.LIN_N), (H.GA_AT, H.GAIN_N), (H.GB_AT, H.GAIN_N), (H.OE_AT, H.OE_N)))
    assert np.all(np.diff(lin) >= 0) and np.all(np.diff(ga) >= 0) and np.all(np.diff(oe) >= 0)
    assert np.all(np.diff(gb) <= 0)  # the tone gain EETF(n) / n is the one falling function among them: monotone the other way
    assert lin[0] == 0 and lin[-1] == 1 << 28 and oe[0] == 0 and oe[-1] == 65536
    assert ga[-1] == ga[-2] == 1 << 30 and gb[0] == int(np.floor(s[2] / s[3] * 16777216.0 + 0.5)) and gb[-1] == gb[-2]
    assert abs(int(gb[-1]) - (1 << 24)) <= 1  # the peak lands on the target
    for r in range(3):
        assert got[17 + 3 * r:20 + 3 * r].sum() == 1 << 20
    assert got[14:17].sum() == 65536 and got[29:32].sum() == 0 and got[32:35].sum() == 0


def test_defaults_resolve():
    assert np.array_equal(E.hdr_tables(H.PQ), E.hdr_tables(H.PQ, 0, 1000, 203, 1, 0))
    assert np.array_equal(E.hdr_tables(H.HLG, 0, 0, 0, 5, 0)[8:], E.hdr_tables(H.HLG, 0, 1000, 203, 6, 0)[8:])  # 5 and 6 are one matrix


# ---------------------------------------------------------------- the rule against the model
def sweep(s):
    """every grey, the lattice Y step 7 x Cb step 13 x Cr step 13, 200 000 random triples, 200 000 triples made forwards from in-gamut BT.709 colours"""
    transfer, full, peak = s[0], s[1], s[2]
    rng = np.random.default_rng(22)
    g = np.arange(1024)
    ly, lb, lr = (a.ravel() for a in np.meshgrid(np.arange(0, 1024, 7), np.arange(0, 1024, 13), np.arange(0, 1024, 13), indexing="ij"))
    rnd = rng.integers(0, 1024, (3, 200000))
    # forwards: linear BT.709 RGB at 0.01 .. peak cd/m^2 (log-uniform level, any chromaticity inside the gamut) -> BT.2020 -> the transfer -> codes
    level = np.exp(rng.uniform(np.log(0.01), np.log(float(peak)), 200000))
    rgb709 = rng.uniform(0.0, 1.0, (3, 200000))
    rgb709 = rgb709 / rgb709.max(axis=0) * level
    rgb2020 = np.linalg.inv(np.array(H.gamut_matrix())) @ rgb709
    if transfer == H.PQ:
        e = H.pq_inv(np.clip(rgb2020, 0.0, 10000.0))
    else:  # invert the OOTF (display -> scene), then the OETF
        yd = H.LUMA2020[0] * rgb2020[0] + H.LUMA2020[1] * rgb2020[1] + H.LUMA2020[2] * rgb2020[2]
        gam = H.hlg_gamma(peak)
        scene = np.clip(rgb2020 / peak * np.power(np.maximum(yd / peak, 1e-12), (1.0 - gam) / gam), 0.0, 1.0)
        e = np.where(scene <= 1.0 / 12.0, np.sqrt(3.0 * scene), H.HLG_A * np.log(np.maximum(12.0 * scene - H.HLG_B, 1e-12)) + H.HLG_C)
    ey = H.KR * e[0] + (1.0 - H.KR - H.KB) * e[1] + H.KB * e[2]
    eb, er = (e[2] - ey) / (2.0 * (1.0 - H.KB)), (e[0] - ey) / (2.0 * (1.0 - H.KR))
    fy, fb, fr = (ey * 1023, eb * 1023 + 512, er * 1023 + 512) if full else (ey * 876 + 64, eb * 896 + 512, er * 896 + 512)
    fwd = [np.clip(np.floor(v + 0.5), 0, 1023).astype(np.int64) for v in (fy, fb, fr)]
    return (np.concatenate([g, ly, rnd[0], fwd[0]]), np.concatenate([np.full(1024, 512), lb, rnd[1], fwd[1]]), np.concatenate([np.full(1024, 512), lr, rnd[2], fwd[2]]))


@pytest.mark.parametrize("s", SETS, ids=IDS)
def test_rule_is_within_one_code_of_the_model_and_fits_its_types(s):
    y, cb, cr = sweep(s)
    shadow = H.Shadow()
    got = H.rule_out(E.hdr_tables(*s), y, cb, cr, shadow)
    want = H.model_out(s[4], s[5], *H.model_rgb(s[0], s[1], s[2], s[3], y, cb, cr))
    for name, a, b in zip(("Y'", "Cb", "Cr"), got, want):
        d = np.abs(a - np.clip(b, 0.0, 255.0))
        print("%s: max %.4f mean %.4f" % (name, d.max(), d.mean()))
        # The bound is a design condition on the fixed-point widths: rounding to a code costs up to 0.5, the rule's own error must stay below the other 0.5.
        # Measured over this sweep, all eight parameter sets: max 0.520 / 0.516 / 0.516, largest mean 0.30 / 0.25 / 0.24 codes (Y' / Cb / Cr).
        assert d.max() <= 1.0, (name, float(d.max()), [int(v[np.argmax(d)]) for v in (y, cb, cr)])
    # every intermediate fits the integer type section 22 names for it (numpy int64 shadows of the same arithmetic)
    assert set(shadow.peak) >= {"t", "x", "lin_prod", "l", "gain_prod", "gain", "v", "w_prod", "w", "u_sum", "u", "oe_prod", "e", "y_sum", "c_sum"}
    assert all(shadow.fits().values()), {k: (v, H.Shadow.TYPES[k]) for k, v in shadow.peak.items() if not shadow.fits()[k]}


def test_a_flat_area_is_what_the_picture_path_gives():
    """tone_map_nv12 (what the device is compared with) and rule_out (what the model is compared with) are one rule"""
    blk = E.hdr_tables(H.HLG)
    y10, c10 = np.full((4, 4), 700), np.stack([np.full((2, 2), 400), np.full((2, 2), 600)], 2).reshape(2, 4)
    planes = [np.ascontiguousarray((p << 6).astype("<u2")).view(np.uint8).reshape(p.shape[0], -1) for p in (y10, c10)]
    oy, ouv = H.tone_map_nv12(blk, H.FMT_P010, planes, 4, 4)
    want = H.rule_out(blk, np.array([700]), np.array([400]), np.array([600]))
    assert np.all(oy == want[0][0]) and np.all(ouv[:, 0::2] == want[1][0]) and np.all(ouv[:, 1::2] == want[2][0])


# ---------------------------------------------------------------- arguments
def test_hdr_tables_arguments():
    L, n = E.load(), C.c_size_t(0)
    buf = np.zeros(H.BLOCK_WORDS, np.int32)
    p = buf.ctypes.data_as(C.c_void_p)
    ok = (16, 0, 0, 0, 1, 0)
    assert L.mi355enc_hdr_tables(*ok, None, 0, C.byref(n)) == 0 and n.value == H.BLOCK_WORDS  # the size alone
    assert L.mi355enc_hdr_tables(*ok, p, H.BLOCK_WORDS - 1, C.byref(n)) == E.ERR_OVERFLOW and not buf.any()
    assert L.mi355enc_hdr_tables(*ok, p, H.BLOCK_WORDS, None) == E.ERR_ARG
    for bad in ((1, 0, 0, 0, 1, 0), (17, 0, 0, 0, 1, 0), (16, 2, 0, 0, 1, 0), (16, -1, 0, 0, 1, 0), (16, 0, 399, 0, 1, 0), (16, 0, 10001, 0, 1, 0), (18, 0, 2001, 0, 1, 0),
                (16, 0, 0, 99, 1, 0), (16, 0, 0, 401, 1, 0), (16, 0, 0, 0, 2, 0), (16, 0, 0, 0, 9, 0), (16, 0, 0, 0, 0, 0), (16, 0, 0, 0, 1, 2)):
        assert L.mi355enc_hdr_tables(*bad, p, H.BLOCK_WORDS, C.byref(n)) == E.ERR_ARG, bad
        with pytest.raises(E.EncoderError):
            E.hdr_tables(*bad)
    for good in ((16, 0, 400, 100, 5, 1), (16, 1, 10000, 400, 6, 0), (18, 0, 2000, 400, 1, 1), (18, 1, 400, 100, 1, 0)):
        assert L.mi355enc_hdr_tables(*good, p, H.BLOCK_WORDS, C.byref(n)) == 0, good
    assert L.mi355enc_set_hdr_input(None, 16, 0, 0, 0) == E.ERR_ARG  # (no handle: the state checks need a device, tests/test_hdr_gpu.py)
