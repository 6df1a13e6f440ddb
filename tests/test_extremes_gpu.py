"""GPU parity at the arithmetic limits: the kernels against the CPU oracle, bit-exact, on saturated full-range content -- SADs at the top of their u16
lanes, the quantiser's level clamp, the six-tap filter's clips and the limits of its intermediates, plane prediction past the rails, the deblocking filter
at 0 / 255, adaptive quantisation at both ends.  tests/test_extremes_cpu.py asserts on the oracle that these inputs (tests/extremes.py) reach those
branches.  All calls go through the C ABI (include/mi355enc.h) via ceracoder_amd.enc; small geometries only, many inputs per encoder."""
import numpy as np
import pytest

from tests import extremes as X
from tests.util import db_picture_sat, first_diff, random_records

pytestmark = pytest.mark.gpu

IMV_FIELDS = ("mvx", "mvy", "sad", "bits")
PMB_FIELDS = ("mvx", "mvy", "mb_type", "i16_mode", "chroma_mode", "qp", "nzmask", "cost")
FAMILIES = {"sat": X.SAT_KINDS, "stripes": X.STRIPE_KINDS, "shift": X.SHIFT_KINDS}


def _coded(w, h):
    return (w + 15) // 16 * 16, (h + 15) // 16 * 16


def _same(dev, orc, what):
    assert np.array_equal(dev, orc), (what, first_diff(dev, orc))


def _same_fields(dev, orc, fields, what):
    for f in fields:
        assert np.array_equal(dev[f], orc[f]), (what, f, first_diff(dev[f], orc[f]))


def _same_picture(dev, orc, fields, what):
    """(rec_y, rec_uv, records, levels) of a stage"""
    _same_fields(dev[2], orc[2], fields, what)
    _same(dev[3], orc[3], what + ("levels",))
    _same(dev[0], orc[0], what + ("luma",))
    _same(dev[1], orc[1], what + ("chroma",))


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("family", ["sat", "stripes", "shift"])
def test_search_at_the_limits(E, oracle, w, h, family):
    """stage_me + three stage_me_select iterations: every SAD of the +-16 window (65 280 on the blocks of 16), the first selection and the Jacobi passes;
    the winner in the corner of the window on the shifted pairs, nothing but ties on the stripes."""
    W, H = _coded(w, h)
    e = E.Encoder(W, H, fixed_qp=30)
    for kind in FAMILIES[family]:
        (cy, _), (ry, _) = X.pair(kind, w, h)
        for qp in (X.QPS if family != "stripes" else [0, 51]):
            d_surf, d_imv = e.stage_me(cy, ry, qp)
            o_surf, o_imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
            _same(d_surf[:, :33, :33], o_surf.reshape(-1, 33, 33), (kind, qp, "surface"))
            _same_fields(d_imv, o_imv, IMV_FIELDS, (kind, qp, "first selection"))
            for it in range(3):
                o_imv = oracle.me_select(o_surf, o_imv, W // 16, H // 16, 16, qp, threads=8)
                d_imv = e.stage_me_select(d_surf, d_imv, qp)
                _same_fields(d_imv, o_imv, IMV_FIELDS, (kind, qp, "selection pass", it))
    e.close()


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("family", ["stripes", "shift"])
def test_refinement_at_the_limits(E, oracle, w, h, family):
    """stage_subpel: half and quarter samples of references whose six-tap planes clip on both sides (stripes), and around a winner in the corner of the
    window, beyond it and beyond the picture border (shifted pairs) -- vectors and costs."""
    W, H = _coded(w, h)
    e = E.Encoder(W, H, fixed_qp=30)
    for kind in FAMILIES[family]:
        (cy, _), (ry, _) = X.pair(kind, w, h)
        for qp in X.QPS:
            mbi = oracle.imv_to_mbinfo(X.settled_field(oracle, kind, w, h, qp)[1], qp)
            orc = oracle.subpel_frame(cy, ry, mbi, qp, threads=8)
            dev = e.stage_subpel(cy, ry, mbi, qp)
            _same_fields(dev, orc, ("mvx", "mvy", "cost"), (kind, qp))
    e.close()


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("t8", [False, True])
def test_inter_stage_at_the_limits(E, oracle, w, h, t8):
    """stage_inter (the two-kernel form) with and without the refinement, 4x4 and 8x8 transform: prediction from saturated references, residuals of +-255 over
    whole blocks through the quantiser's clamp at QP 0, reconstruction clipped at both rails."""
    W, H = _coded(w, h)
    e = E.Encoder(W, H, fixed_qp=30, transform8x8=t8)
    plan = [(k, q) for k in X.SAT_KINDS for q in (X.QPS if not t8 else [0, 30])] + [(k, q) for k in X.STRIPE_KINDS for q in ([0, 30] if not t8 else [5])] \
        + [(k, q) for k in X.SHIFT_KINDS[::3] for q in [6, 51]]
    with X.oracle_mode(oracle, t8=t8):
        for kind, qp in plan:
            (cy, cuv), (ry, ruv) = X.pair(kind, w, h)
            mbi = oracle.imv_to_mbinfo(X.settled_field(oracle, kind, w, h, qp)[1], qp)
            for sub in (False, True):
                m = oracle.subpel_frame(cy, ry, mbi, qp, threads=8) if sub else mbi
                orc = oracle.inter_frame(cy, cuv, ry, ruv, m, qp)
                dev = e.stage_inter(cy, cuv, ry, ruv, m, qp)
                _same_picture(dev, orc, ("mvx", "mvy", "mb_type", "qp", "nzmask"), (kind, qp, sub))
    e.close()


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("variant", ["plain", "refine", "refine+intra", "partitions", "partitions+intra", "t8"])
def test_fused_p_stage_at_the_limits(E, oracle, w, h, variant):
    """stage_pmb (+ the intra macroblocks it decided): skip probe, refinement, intra-or-inter, residual -- refine off and on, with and without intra
    decisions, with partitions, with the 8x8 transform; records, levels and both reconstruction planes."""
    W, H = _coded(w, h)
    refine, intra, part, t8 = variant != "plain", variant.endswith("intra") or variant == "t8", variant.startswith("partitions"), variant == "t8"
    e = E.Encoder(W, H, fixed_qp=30, partitions=part, transform8x8=t8)
    full = variant == "refine+intra"  # the whole cross of content and QP once; two QPs elsewhere
    plan = [(k, q) for k in X.SAT_KINDS for q in (X.QPS if full else [0, 30])] + [(k, q) for k in X.STRIPE_KINDS for q in ([0, 51] if full else [6])] \
        + [(k, q) for k in X.SHIFT_KINDS for q in ([5, 30] if full else [51])]
    with X.oracle_mode(oracle, t8=t8, part=part):
        for kind, qp in plan:
            (cy, cuv), (ry, ruv) = X.pair(kind, w, h)
            surf, imv = X.settled_field(oracle, kind, w, h, qp)
            idec = oracle.intra_decide(oracle.intra_analyse(cy, cuv), W // 16, H // 16, qp, False) if intra else None
            orc = oracle.pmb_frame(cy, cuv, ry, ruv, imv, surf, qp, refine=refine, idec=idec, threads=8)[:4]
            dev = e.stage_pmb(cy, cuv, ry, ruv, imv, oracle.surf_to_device(surf), qp, refine=refine, idec=idec)
            _same_picture(dev, orc, PMB_FIELDS, (kind, qp))
    e.close()


def _intra_contents(w, h):
    return [(k, X.pair(k, w, h)[0]) for k in X.SAT_KINDS] + [(("ramps",), X.ramps(w, h))] + [(k, X.pair(k, w, h)[1]) for k in X.STRIPE_KINDS]


# (intra_mode, i4x4, i8x8 with the 8x8 transform, slice rows, [(QP, drop)] or None: every QP)
INTRA_VARIANTS = {
    "rows": (0, True, False, 0, None), "diagonals": (1, True, False, 0, None), "bands": (2, True, False, 0, None),
    "i16-only": (0, False, False, 0, [(0, 0), (30, 0)]), "i8x8": (0, True, True, 0, [(0, 0), (5, 0), (30, 0)]),
    "rows-sliced": (0, True, False, 2, [(0, 0), (30, 0)]), "diagonals-sliced": (1, True, False, 2, [(6, 0)]), "bands-sliced": (2, False, False, 2, [(6, 0)]),
    "drop": (0, True, False, 0, [(51, 4)]), "diagonals-drop": (1, True, False, 0, [(51, 4)]), "bands-drop": (2, True, False, 0, [(51, 4)]),
}


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("variant", list(INTRA_VARIANTS))
def test_intra_stage_at_the_limits(E, oracle, w, h, variant):
    """stage_intra_analyse and stage_intra on blocks of 0 / 255, ramps into the rails and stripes: every candidate's SAD and the decisions (plane prediction
    clipping at both ends), then records, levels and reconstruction -- the three schedules, Intra_4x4 on and off, Intra_8x8 with the 8x8 transform, slices of
    two macroblock rows, rate control's drop level 4 at QP 51."""
    W, H = _coded(w, h)
    imode, i4, i8, rows, ops = INTRA_VARIANTS[variant]
    e = E.Encoder(W, H, fixed_qp=30, i4x4=i4, intra_mode=imode, transform8x8=i8, i8x8=i8)
    e.stage_set_slice_rows(rows)
    with X.oracle_mode(oracle, t8=i8, i8=i8, i4=i4, slice_rows=rows):
        for kind, (cy, cuv) in _intra_contents(w, h):
            for qp, drop in (ops or [(q, 0) for q in X.QPS]):
                if not i8 and not drop:
                    (d_sad, d_dec), o_sad = e.stage_intra_analyse(cy, cuv, qp), oracle.intra_analyse(cy, cuv)
                    _same(d_sad, o_sad, (kind, qp, "candidate SADs"))
                    _same_fields(d_dec, oracle.intra_decide(o_sad, W // 16, H // 16, qp, i4), ("mode16", "cmode", "use_i4", "cost", "cost_luma", "modes4"), (kind, qp, "decisions"))
                orc = oracle.intra_frame(cy, cuv, qp, drop)
                dev = e.stage_intra(cy, cuv, qp, drop)
                _same_picture(dev, orc, ("mb_type", "i16_mode", "chroma_mode", "cost", "qp", "nzmask", "mvx", "mvy"), (kind, qp, drop))
    e.close()


@pytest.mark.parametrize("mbw,mbh", [(1, 1), (4, 3), (11, 9)])
@pytest.mark.parametrize("mode", [0, 1])
def test_deblocking_at_the_rails(E, oracle, mbw, mbh, mode):
    """stage_deblock (band kernel and per-diagonal form) on db_picture_sat with random_records -- QPs 10 .. 51 and 40 .. 51, with and without NZ_T8 -- against
    oracle.deblock_frame: p0 + delta and q0 - delta clipped at 0 and at 255, in luma and in both chroma components."""
    e = E.Encoder(16 * mbw, 16 * mbh, fixed_qp=30, deblock_mode=mode)
    y, uv = db_picture_sat(mbw, mbh, X.SEED_DB)
    for qp in ((10, 51), (40, 51)):
        for t8 in (0.3, 0.0):
            rec = random_records(mbw, mbh, X.SEED_REC, t8=t8, qp=qp)
            o_y, o_uv = oracle.deblock_frame(y, uv, rec)
            d_y, d_uv = e.stage_deblock(y, uv, rec)
            _same(d_y, o_y, (qp, t8, "luma"))
            _same(d_uv, o_uv, (qp, t8, "chroma"))
    e.close()


@pytest.mark.parametrize("w,h", X.GEOMS)
@pytest.mark.parametrize("mode", [0, 1])
def test_deblocking_of_coded_saturated_pictures(E, oracle, w, h, mode):
    """... and on the oracle's own pre-filter pictures and records of a sat_blocks I picture and P picture at QP 44 and 51."""
    W, H = _coded(w, h)
    e = E.Encoder(W, H, fixed_qp=30, deblock_mode=mode)
    (cy, cuv), (ry, ruv) = X.sat_pair(w, h, 16)
    for qp in (44, 51):
        oe = oracle.Encoder(w, h, gop=60, threads=8, scenecut=False)
        for y, uv in ((ry, ruv), (cy, cuv)):
            oe.encode(y[:h, :w], uv[:h // 2, :w], qp)
            d_y, d_uv = e.stage_deblock(oe.prefilter_y, oe.prefilter_uv, oe.mbinfo)
            _same(d_y, oe.recon_y, (qp, "luma"))
            _same(d_uv, oe.recon_uv, (qp, "chroma"))
        oe.close()
    e.close()


@pytest.mark.parametrize("w,h", X.STREAM_GEOMS)
@pytest.mark.parametrize("cfg", list(X.STREAM_CFGS))
def test_saturated_streams_equal_oracle(E, oracle, w, h, cfg):
    """sat_clip, six pictures, QPs 0, 51, 3, 26, 6, 40, an IDR picture every third: Constrained Baseline; what speed-preset 2 selects (8x8 transform,
    Intra_8x8, adaptive quantisation); partitions; the library's default configuration (sliced P pictures, slice-local deblocking); one and three pictures in
    flight on a device of its own.  Access units and both reconstruction planes equal the oracle's picture by picture, the independent decoder reproduces
    them, no access unit outgrows mi355enc_max_au_bytes, and nothing was recovered from."""
    kw, mode, _ = X.STREAM_CFGS[cfg]
    depth = kw.get("pipeline_depth", 0)
    want = X.oracle_stream(oracle, w, h, cfg)
    with X.oracle_mode(oracle, **mode):  # (the library reads nothing of the oracle's; this keeps the two in the same state for a reader)
        e = E.Encoder(w, h, gop=X.STREAM_GOP, fixed_qp=30, scenecut=False, **kw)
    assert e._out.size == X.max_au_bytes(w, h)
    if cfg == "lib":
        assert e.p_slice_rows == e.slice_rows == oracle.slice_rows_for((h + 15) // 16, oracle.auto_slices((h + 15) // 16), True)
    dec = oracle.Decoder()
    got = []
    for i, (y, uv) in enumerate(X.stream_clip(w, h)):
        e.set_fixed_qp(X.STREAM_QPS[i % len(X.STREAM_QPS)])
        e.submit(y, uv, pts=i)
        if e.pending > depth:
            got.append(e.collect()[:3])
            if depth == 0:
                _same(e.fetch(E.FETCH_RECON_Y), want[i][2], (cfg, i, "luma"))
                _same(e.fetch(E.FETCH_RECON_UV), want[i][3], (cfg, i, "chroma"))
    while e.pending:
        got.append(e.collect()[:3])
    for i, (au, key, pts) in enumerate(got):
        assert (key, pts) == (want[i][1], i)
        assert au == want[i][0], (cfg, "access unit", i, len(au), len(want[i][0]))
        assert len(au) <= X.max_au_bytes(w, h)
        dy, duv = dec.decode(au)
        _same(dy, want[i][2], (cfg, i, "decoded luma"))
        _same(duv, want[i][3], (cfg, i, "decoded chroma"))
    _same(e.fetch(E.FETCH_RECON_Y), want[-1][2], (cfg, "last luma"))
    _same(e.fetch(E.FETCH_RECON_UV), want[-1][3], (cfg, "last chroma"))
    assert e.stats().recoveries == 0
    e.close()
