"""GPU parity over the accepted size range (mi355enc_open: even sizes from 16 to 8192 per axis): strips of 8192 columns or 8192 rows, every remainder of the
per-workgroup groupings, the macroblock counts at which the hand-over picks another kernel, and the input-side kernels at the longest rows and columns.
tests/test_size_range_cpu.py asserts on the oracle that these inputs (tests/sizerange.py) carry intra, coded, refined and skipped macroblocks at the far end
of the strips.  Everything is integer: every comparison is ==.  Besides the outputs every stream test asserts a zero error word and no recovery: the kernels
that wait for each other on the device do so under a bound, and a bound that 128 deblocking bands or 512 intra rows cannot meet shows there first."""
import numpy as np
import pytest

from tests import extremes as X
from tests import sizerange as S
from tests.util import first_diff

pytestmark = pytest.mark.gpu

IMV_FIELDS = ("mvx", "mvy", "sad", "bits")
PMB_FIELDS = ("mvx", "mvy", "mb_type", "i16_mode", "chroma_mode", "qp", "nzmask", "cost")
INTRA_FIELDS = ("mb_type", "i16_mode", "chroma_mode", "cost", "qp", "nzmask", "mvx", "mvy")


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
    _same(dev[3], orc[3], (what, "levels"))
    _same(dev[0], orc[0], (what, "luma"))
    _same(dev[1], orc[1], (what, "chroma"))


def _no_trouble(e, what=None):
    """as tests/test_longrun_gpu.py reads them: nothing was recovered from, and no bounded wait on the device ran out"""
    st = e.stats()
    assert st.recoveries == 0 and st.last_error_word == 0 and e.error_word() == 0, (what, st.recoveries, st.last_error_word, e.error_word())


# ---------------------------------------------------------------- 3. the stage kernels on strips: picture 1 against picture 0 of strip_clip
@pytest.mark.parametrize("w,h", S.STRIPS)
def test_search_on_strips(E, oracle, w, h):
    """stage_me and three stage_me_select passes against the oracle, and the sparse pass (a wave checks eight macroblocks) against the dense one."""
    W, H = _coded(w, h)
    (cy, _), (ry, _) = S.strip_pair(w, h)
    o_surf, fields = S.settled_field(oracle, w, h, S.STRIP_QP)
    e = E.Encoder(W, H, fixed_qp=S.STRIP_QP)
    try:
        d_surf, d_imv = e.stage_me(cy, ry, S.STRIP_QP)
        _same(d_surf[:, :33, :33], o_surf.reshape(-1, 33, 33), "surfaces")
        _same_fields(d_imv, fields[0], IMV_FIELDS, "first selection")
        prev, copied = None, 0
        for it in range(3):
            nxt = e.stage_me_select(d_surf, d_imv, S.STRIP_QP)
            _same_fields(nxt, fields[it + 1], IMV_FIELDS, ("selection pass", it))
            if prev is not None:
                sparse = e.stage_me_select_next(d_surf, d_imv, prev, S.STRIP_QP)
                _same_fields(sparse, nxt, IMV_FIELDS, ("sparse pass", it))
                copied += int((sparse == d_imv).sum())
            prev, d_imv = d_imv, nxt
        assert copied > 0
        _no_trouble(e)
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.STRIPS)
def test_refinement_and_inter_stage_on_strips(E, oracle, w, h):
    """stage_subpel, then stage_inter on the refined field (the two-kernel form)."""
    W, H = _coded(w, h)
    (cy, cuv), (ry, ruv) = S.strip_pair(w, h)
    qp = S.STRIP_QP
    mbi = oracle.imv_to_mbinfo(S.settled_field(oracle, w, h, qp)[1][-1], qp)
    o_sub = oracle.subpel_frame(cy, ry, mbi, qp, threads=8)
    e = E.Encoder(W, H, fixed_qp=qp)
    try:
        _same_fields(e.stage_subpel(cy, ry, mbi, qp), o_sub, ("mvx", "mvy", "cost"), "refinement")
        assert (o_sub["mvx"] % 4 != 0).any() or (o_sub["mvy"] % 4 != 0).any()
        _same_picture(e.stage_inter(cy, cuv, ry, ruv, o_sub, qp), oracle.inter_frame(cy, cuv, ry, ruv, o_sub, qp), ("mvx", "mvy", "mb_type", "qp", "nzmask"), "inter")
        _no_trouble(e)
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.STRIPS)
@pytest.mark.parametrize("part", [False, True])
def test_fused_p_stage_on_strips(E, oracle, w, h, part):
    """stage_pmb with the intra decisions and the intra macroblocks it decided (intra_p_row: the row's bit sets up to column 511), at QP 30, at QP 51 on
    the drop ladder and at QP 0; once more with partitions."""
    W, H = _coded(w, h)
    (cy, cuv), (ry, ruv) = S.strip_pair(w, h)
    e = E.Encoder(W, H, fixed_qp=S.STRIP_QP, partitions=part)
    try:
        with X.oracle_mode(oracle, part=part):
            for qp, drop in (S.PMB_POINTS if not part else S.PMB_POINTS[:1]):
                surf, fields = S.settled_field(oracle, w, h, qp)
                idec = oracle.intra_decide(oracle.intra_analyse(cy, cuv), W // 16, H // 16, qp, False)
                orc = oracle.pmb_frame(cy, cuv, ry, ruv, fields[-1], surf, qp, drop=drop, refine=True, idec=idec, threads=8)[:4]
                dev = e.stage_pmb(cy, cuv, ry, ruv, fields[-1], oracle.surf_to_device(surf), qp, drop=drop, refine=True, idec=idec, run_intra_p=True)
                _same_picture(dev, orc, PMB_FIELDS, (qp, drop))
                if qp == S.STRIP_QP:
                    g = orc[2].reshape(H // 16, W // 16)
                    g = g if S.is_wide(w, h) else g.T
                    assert (g["mb_type"][:, -1] != 1).any(), "no intra macroblock at the far end"
        _no_trouble(e)
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.STRIPS)
def test_intra_analysis_on_strips(E, oracle, w, h):
    W, H = _coded(w, h)
    cy, cuv = S.strip_pair(w, h)[0]
    qp = S.STRIP_QP
    o_sad = oracle.intra_analyse(cy, cuv)
    e = E.Encoder(W, H, fixed_qp=qp)
    try:
        d_sad, d_dec = e.stage_intra_analyse(cy, cuv, qp)
        _same(d_sad, o_sad, "candidate SADs")
        _same_fields(d_dec, oracle.intra_decide(o_sad, W // 16, H // 16, qp, True), ("mode16", "cmode", "use_i4", "cost", "cost_luma", "modes4"), "decisions")
    finally:
        e.close()


_intra = {}


def _oracle_intra(oracle, w, h, i8):
    if (w, h, i8) not in _intra:
        cy, cuv = S.strip_pair(w, h)[0]
        with X.oracle_mode(oracle, t8=i8, i8=i8):
            _intra[(w, h, i8)] = oracle.intra_frame(cy, cuv, S.STRIP_QP)
    return _intra[(w, h, i8)]


@pytest.mark.parametrize("w,h", S.STRIPS)
@pytest.mark.parametrize("variant", ["rows", "diagonals", "bands", "i8x8"])
def test_intra_stage_on_strips(E, oracle, w, h, variant):
    """stage_intra under the three schedules (a workgroup per macroblock row: 512 rows waiting for each other, or one row of 512; a launch per anti-diagonal;
    the lock-step bands) and with Intra_8x8."""
    W, H = _coded(w, h)
    cy, cuv = S.strip_pair(w, h)[0]
    i8 = variant == "i8x8"
    orc = _oracle_intra(oracle, w, h, i8)
    e = E.Encoder(W, H, fixed_qp=S.STRIP_QP, intra_mode={"rows": 0, "diagonals": 1, "bands": 2, "i8x8": 0}[variant], transform8x8=i8, i8x8=i8)
    try:
        _same_picture(e.stage_intra(cy, cuv, S.STRIP_QP), orc, INTRA_FIELDS, variant)
        if i8:
            assert ((orc[2]["mb_type"] == 2) & ((orc[2]["nzmask"] >> 27) & 1).astype(bool)).any(), "no Intra_8x8 macroblock"
        _no_trouble(e)
    finally:
        e.close()


_prefilter = {}


def _oracle_prefilter(oracle, w, h):
    """[(pre-filter luma, chroma, records, deblocked luma, chroma)] of the IDR and the first P picture of strip_clip at QP 30"""
    if (w, h) not in _prefilter:
        oe = oracle.Encoder(w, h, gop=60, threads=8, scenecut=False)
        out = []
        for y, uv in S.strip_clip(w, h)[:2]:
            oe.encode(y, uv, S.STRIP_QP)
            out.append((oe.prefilter_y, oe.prefilter_uv, oe.mbinfo, oe.recon_y, oe.recon_uv))
        oe.close()
        _prefilter[(w, h)] = out
    return _prefilter[(w, h)]


@pytest.mark.parametrize("w,h", S.STRIPS)
@pytest.mark.parametrize("mode", [0, 1])
def test_deblocking_on_strips(E, oracle, w, h, mode):
    """stage_deblock on the oracle's pre-filter pictures and records of an I and a P picture: 128 bands of one to nine macroblocks, or one to three bands of 512
    (the P picture's walked in two parts, cut near column 256)."""
    W, H = _coded(w, h)
    e = E.Encoder(W, H, fixed_qp=S.STRIP_QP, deblock_mode=mode)
    try:
        for i, (py, puv, rec, ry, ruv) in enumerate(_oracle_prefilter(oracle, w, h)):
            d_y, d_uv = e.stage_deblock(py, puv, rec)
            _same(d_y, ry, (i, "luma"))
            _same(d_uv, ruv, (i, "chroma"))
        _no_trouble(e)
    finally:
        e.close()


# ---------------------------------------------------------------- 4. whole streams on strips
def _run_stream(E, oracle, w, h, kw, want, clip, qps, gop, what):
    """the clip through an encoder; access units, key flags, the reconstruction (picture by picture at depth 0), the independent decoder on the device's access
    units, the error word and the recovery count"""
    depth = kw.get("pipeline_depth", 0)
    e = E.Encoder(w, h, gop=gop, fixed_qp=30, scenecut=False, **kw)
    try:
        got = []
        for i, (y, uv) in enumerate(clip):
            e.set_fixed_qp(qps[i % len(qps)])
            e.submit(y, uv, pts=i)
            if e.pending > depth:
                got.append(e.collect()[:3])
                if depth == 0:
                    _same(e.fetch(E.FETCH_RECON_Y), want[i][2], (what, i, "luma"))
                    _same(e.fetch(E.FETCH_RECON_UV), want[i][3], (what, i, "chroma"))
        while e.pending:
            got.append(e.collect()[:3])
        dec = oracle.Decoder()
        for i, (au, key, pts) in enumerate(got):
            assert (key, pts) == (want[i][1], i), (what, i)
            assert au == want[i][0], (what, "access unit", i, len(au), len(want[i][0]))
            dy, duv = dec.decode(au)
            _same(dy, want[i][2], (what, i, "decoded luma"))
            _same(duv, want[i][3], (what, i, "decoded chroma"))
        assert dec.size == (w, h)
        dec.close()
        _same(e.fetch(E.FETCH_RECON_Y), want[-1][2], (what, "last luma"))
        _same(e.fetch(E.FETCH_RECON_UV), want[-1][3], (what, "last chroma"))
        _no_trouble(e, what)
        return e.slice_rows, e.p_slice_rows, e.debug_get_counters()
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.STRIPS)
@pytest.mark.parametrize("cfg", list(S.STREAM_CFGS))
def test_strip_streams_equal_oracle(E, oracle, w, h, cfg):
    """Five pictures of strip_clip, an IDR picture every third, QPs 0, 51, 3, 26, 6: every toolset of extremes.STREAM_CFGS, Intra_4x4 in P pictures, and adaptive
    quantisation with three slices (the QP_Y chain once per slice)."""
    want = S.strip_stream(oracle, cfg, w, h)
    rows = _run_stream(E, oracle, w, h, S.enc_args(S.STREAM_CFGS, cfg, h), want, S.strip_clip(w, h), X.STREAM_QPS, S.STREAM_GOP, cfg)
    mbw, mbh = S.mb_size(w, h)
    if cfg == "depth2":
        # Three pictures in flight on a device of its own: the fused P stage is gated and counts mbw macroblocks into every row's word per P picture (tests/test_longrun_gpu.py,
        # _bookings) -- unless the picture's deblocking launch would take more than three quarters of the compute units (a workgroup per band and plane and, at up to 3600
        # macroblocks, one per intra row: S.wait_wgs), where nothing waits on the device and the pictures are coded in stream order ("Size range")
        n_p = sum(not s[1] for s in want)
        assert rows[2]["pmb_rows_total"] == (mbw * n_p if S.wait_wgs(mbw, mbh) <= S.WAIT_WGS_MAX else 0), (rows[2], S.wait_wgs(mbw, mbh))
    if cfg == "lib":
        assert rows[0] == rows[1] == oracle.slice_rows_for(mbh, oracle.auto_slices(mbh), True)
    if cfg == "aq-sliced":
        assert rows[0] == rows[1] == oracle.slice_rows_for(mbh, min(3, mbh), False) and (rows[0] > 0) == (mbh > 1)
        assert len(set(int(q) for s in want for q in np.unique(s[4]["qp"]))) > len(X.STREAM_QPS[:S.STREAM_N]), "adaptive quantisation moved no QP"


@pytest.mark.parametrize("w,h", S.REFRESH_STRIPS)
@pytest.mark.parametrize("depth", [0, 2])
def test_intra_refresh_on_strips(E, oracle, w, h, depth):
    """Periodic intra refresh with a cycle of three pictures -- 171 forced columns per picture of the wide strip, one or two of the tall one's three -- held to
    tests/irref.py as tests/test_intra_refresh_gpu.py holds it: the schedule, the forced columns, the vectors left of them, and the independent decoder."""
    from tests.test_intra_refresh_gpu import _check_structure, _encode, _open
    n, npic = 3, 1 + 2 * 3 + 1
    e = _open(E, w, h, n, qp=S.STRIP_QP, depth=depth, slices=1)
    try:
        aus, keys, drops, recs = _encode(e, S.strip_clip(w, h), npic, depth, fetch=True)
        mbw, mbh = e.mbw, e.mbh
        _no_trouble(e)
    finally:
        e.close()
    _check_structure(aus, keys, drops, ["idr"] + ["p"] * (npic - 1), mbw, mbh, n, oracle, recs, depth)


# ---------------------------------------------------------------- 5. every grouping remainder
def _sweep(E, oracle, cfg, cells):
    for mbw, mbh in cells:
        w, h = S.grid_size(mbw, mbh)
        _run_stream(E, oracle, w, h, S.GRID_CFGS[cfg][0], S.grid_stream(oracle, cfg, mbw, mbh), S.grid_clip(w, h), [S.GRID_QP], 60, (cfg, w, h))


@pytest.mark.parametrize("mbh", list(S.GRID))
@pytest.mark.parametrize("cfg", ["baseline-depth0", "lib-depth2"])
def test_every_remainder_of_the_groupings(E, oracle, cfg, mbh):
    """mbw 1 .. 9 at this mbh, the visible size 2 short of the coded size: four macroblocks per search workgroup, four waves per workgroup of the select, pack
    and aq kernels, eight macroblocks per wave of the sparse pass, two rows per intra band, four per deblocking band, slices rounded to bands, the row-parallel
    writer -- Baseline alone on the device, and the library's defaults with three pictures in flight."""
    _sweep(E, oracle, cfg, [(mbw, mbh) for mbw in S.GRID])


@pytest.mark.parametrize("mbh", list(S.GRID))
def test_remainders_with_preset2_and_aq(E, oracle, mbh):
    """8x8 transform, Intra_8x8 and adaptive quantisation over the diagonal and the first and last row and column of the grid."""
    _sweep(E, oracle, "preset2-aq", [c for c in S.grid_cells("frame") if c[1] == mbh])


# ---------------------------------------------------------------- 6. the hand-over's thresholds
@pytest.mark.parametrize("w,h", S.THRESHOLDS)
@pytest.mark.parametrize("cfg", list(S.THRESHOLD_CFGS))
def test_scan_and_chain_thresholds(E, oracle, w, h, cfg):
    """IDR + P at the macroblock counts where levels_scan_kernel changes its instantiation (4096 / 8192 / 32768: the last size of one, the first of the next), with
    adaptive quantisation also qp_chain_kernel at up to 33 macroblocks per thread."""
    _run_stream(E, oracle, w, h, S.THRESHOLD_CFGS[cfg][0], S.threshold_stream(oracle, cfg, w, h), S.threshold_clip(w, h), [S.THRESHOLD_QP], 60, cfg)


# ---------------------------------------------------------------- 8. the input-side kernels at the longest rows and columns
def _same_planes(got, want, what):
    _same(got[0], want[0], (what, "luma"))
    _same(got[1], want[1], (what, "chroma"))


@pytest.mark.parametrize("w,h", S.INPUT_SHAPES)
def test_conversion_kernels_at_the_extremes(E, w, h):
    """stage_csc, one format of each kernel: YUY2 (csc_planar), BGRx and RGB (csc_rgb), P010, v210 and GRAY8 (csc_deep; v210's 24-sample patch leaves 6 samples
    at 8190 and 8 at 8192) -- and one matrix / range pair of stage_yuv_convert."""
    from oracle import csc as OC
    from tests import cscref as CR
    from tests import yuvref as YR
    from tests.test_yuv_convert_gpu import PAIRS, coef_of, noise
    assert (8190 % 24, 8192 % 24) == (6, 8)
    e = E.Encoder(w, h, fixed_qp=30)
    try:
        for fmt, ref in ((OC.FMT_YUY2, OC), (CR.FMT_BGRX, CR), (CR.FMT_RGB, CR), (YR.FMT_P010, YR), (YR.FMT_V210, YR), (YR.FMT_GRAY8, YR)):
            planes = [np.ascontiguousarray(p) for p in (YR if ref is YR else CR).random_planes(fmt, w, h, np.random.default_rng(fmt * 100 + w))]
            _same_planes(e.stage_csc(fmt, planes), ref.to_nv12(fmt, planes, w, h), ("format", fmt))
    finally:
        e.close()
    pair = PAIRS["full601-lim709"]
    e = E.Encoder(w, h, fixed_qp=30, colorimetry=pair[1], input_colorimetry=pair[0])
    try:
        y, uv = noise(w, h, w)
        _same_planes(e.stage_yuv_convert(y, uv), YR.convert(y, uv, coef_of(pair)), "yuv convert")
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.INPUT_SHAPES)
def test_orientation_at_the_extremes(E, w, h):
    """stage_orient into a coded w x h picture: the two transposing methods 90r and ul-lr (a row of 8192 from a column of 8192 and the other way round) and the
    flip 180."""
    from tests import orientref as OR
    e = E.Encoder(w, h, fixed_qp=30)
    try:
        for m in (E.ORIENT_90R, E.ORIENT_180, E.ORIENT_UL_LR):
            y, uv = OR.noise(*OR.size(m, w, h), 100 * m + w)
            _same_planes(e.stage_orient(m, y, uv), OR.orient_coded(y, uv, m), OR.NAMES[m])
    finally:
        e.close()


@pytest.mark.parametrize("src,dst", [((8192, 128), (1024, 16)), ((8192, 16), (4096, 16))], ids=["8to1", "2to1-across"])
def test_scaling_from_the_widest_input(E, src, dst):
    """stage_scale from 8192 columns: 8 : 1 in both directions (the limit) and 2 : 1 across only."""
    from tests import scaleref as SR
    from tests.test_scale_gpu import planes_of
    e = E.Encoder(dst[0], dst[1], fixed_qp=30, input_size=src)
    try:
        for fmt in (SR.FMT_NV12, SR.FMT_YUY2):
            pl = planes_of(fmt, src[0], src[1], np.random.default_rng(src[1] + fmt))
            _same_planes(e.stage_scale(fmt, pl), SR.to_nv12(fmt, pl, src[0], src[1], dst[0], dst[1]), fmt)
    finally:
        e.close()


def test_letterbox_into_the_widest_target(E):
    """stage_geometry: 2048 x 16 enlarged three times into the middle of 8192 x 64, a border on every side."""
    from tests import geomref as G
    from tests.test_geometry_gpu import planes_of
    insize, dst, target, border = (2048, 16), (1024, 8, 6144, 48), (8192, 64), (37, 201, 90)
    g = E.geometry(insize, dst=dst, border=border)
    assert E.geometry_valid(g, *target) and G.valid(insize[0], insize[1], (0, 0) + insize, dst, *target)
    e = E.Encoder(target[0], target[1], fixed_qp=30, geometry=g)
    try:
        for fmt in (G.FMT_NV12, G.FMT_I420):
            pl = planes_of(fmt, insize[0], insize[1], np.random.default_rng(fmt))
            _same_planes(e.stage_geometry(fmt, pl), G.to_nv12(fmt, pl, insize[0], insize[1], (0, 0) + insize, dst, target[0], target[1], border), fmt)
    finally:
        e.close()


@pytest.mark.parametrize("w,h,scale", [(8192, 32, 1), (64, 8192, 8)])
def test_overlay_on_strips(E, w, h, scale):
    """stage_overlay: a line of 200 characters at the automatic scale -- 1600 columns of the wide strip, and at scale 8 cut off by the tall strip's 64."""
    from tests import overlayref as OV
    from tests.util import pad_planes
    assert OV.auto_scale(h) == scale
    rng = np.random.default_rng(w)
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    py, puv = pad_planes(y, uv)
    text = ("0123456789" * 20)[:200]
    e = E.Encoder(w, h, fixed_qp=30)
    try:
        # (the reference draws on a canvas as wide as the whole line: at scale 8 one style is two seconds of numpy)
        for st in (dict(), dict(halign=0, valign=2, xpad=0, ypad=0, shaded_background=1))[0 if scale == 1 else 1:]:
            got = e.stage_overlay(text, py, puv, **st)
            _same_planes(got, OV.draw_coded(y, uv, text, **st), st)
            assert not np.array_equal(got[0], py)
    finally:
        e.close()


def test_image_layer_of_the_largest_width(E):
    """stage_image: a layer of 4096 x 8 (the widest a layer may be) ending two samples short of the right edge of 8192 x 16."""
    from tests import imageref as IM
    from tests.util import pad_planes
    w, h = 8192, 16
    assert E.IMAGE_MAX_DIM == 4096
    rng = np.random.default_rng(9)
    y, uv = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)
    py, puv = pad_planes(y, uv)
    pix = IM.random_image(rng, 4096, 8)
    e = E.Encoder(w, h, fixed_qp=30)
    try:
        for x, yy, op in ((w - 4096 - 2, 4, 256), (w - 4096 - 1, 3, 77)):
            got = e.stage_image([E.image_layer(IM.to_fmt(pix, E.FMT_RGBX), x, yy, op, E.FMT_RGBX)], py, puv)
            _same_planes(got, IM.blend_coded(y, uv, [IM.layer(pix, x, yy, op)], IM.coefficients(2, 0, w, h)), (x, yy, op))
            assert not np.array_equal(got[0], py)
    finally:
        e.close()


@pytest.mark.parametrize("w,h", S.INPUT_SHAPES)
def test_quality_and_snapshot_kernels_at_the_extremes(E, w, h):
    """stage_quality against tests/qualityref.py (the five integers), stage_snapshot_blocks reduced by 1 and by 8 against tests/snapref.py."""
    from tests import qualityref as Q
    from tests import snapref
    from tests.test_quality_gpu import _with_margin
    rng = np.random.default_rng(w + 3 * h)
    rnd = lambda: (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8))
    a, b = rnd(), rnd()
    e = E.Encoder(w, h, fixed_qp=30)
    try:
        for k, (s, r) in enumerate(((a, a), (a, b))):
            sy, suv = _with_margin(s[0], s[1], w, h, 10 + k)
            ry, ruv = _with_margin(r[0], r[1], w, h, 20 + k)
            want = Q.quality(sy, suv, ry, ruv, w, h)
            q = e.stage_quality(sy, suv, ry, ruv)
            assert q.ints() == want, k
            assert want[4] == (w // 4 - 1) * (h // 4 - 1) and list(q.samples) == [w * h, (w // 2) * (h // 2), (w // 2) * (h // 2)]
        y, uv = snapref.picture(w, h, "noise")
        for s in (1, 8):
            want, qt, (ow, oh) = snapref.levels(y, uv, s, 75)
            got, gqt = e.stage_snapshot_blocks(y, uv, reduce=s, quality=75)
            assert (ow, oh) == E.snapshot_size(w, h, s) and np.array_equal(gqt, qt), s
            for c, (g, x) in enumerate(zip(got, want)):
                _same(g, x, ("still", s, "component", c))
    finally:
        e.close()


def test_element_at_the_widest_caps(tmp_path, E, oracle):
    """mi355h264enc with I420 caps of 8192 x 16, five buffers through the project's probe program: the C ABI's stream of the same pictures, and every access
    unit decodes to that size."""
    import os
    from tests.test_boundary_cpu import PROBE
    if not os.path.exists(PROBE):
        pytest.skip("ceracoder_amd/mi355_gst_probe not built (no GStreamer)")
    from tests.spsref import sps_of
    from tests.test_orient_gst_gpu import _abi, _run
    w, h, n = 8192, 16, 5
    pics = S.strip_clip(w, h)[:n]
    i420 = [[y, np.ascontiguousarray(uv[:, 0::2]), np.ascontiguousarray(uv[:, 1::2])] for y, uv in pics]
    got = _run(tmp_path, "wide", [b"".join(p.tobytes() for p in f) for f in i420], "video/x-raw,format=I420,width=%d,height=%d,framerate=30/1" % (w, h), "")
    assert all((gw, gh) == (w, h) for _, gw, gh in got)
    (s,) = sps_of(got[0][0])
    assert (s["mbw"], s["mbh"]) == (512, 1)
    assert [g[0] for g in got] == _abi(E, w, h, s["colorimetry"], lambda e, i: e.submit_fmt(E.FMT_I420, i420[i], pts=i), n)
    dec = oracle.Decoder()
    for au, _, _ in got:
        dy, _ = dec.decode(au)
        assert dec.size == (w, h) and dy.shape == (16, 8192)
    dec.close()
