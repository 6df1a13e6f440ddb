"""The per-macroblock transform size choice (cfg.transform8x8 = 2) on the device: the fused P stage against its two fixed-transform forms through the rule
of tests/t8ref.py, whole streams through the independent decoder and the oracle's deblocker, schedule invariance, the two-kernel stage's refusal and
the GStreamer element's property."""
import os
import subprocess

import numpy as np
import pytest

from ceracoder_amd import synth
from tests import t8ref
from tests.test_boundary_cpu import HARNESS, gst_env
from tests.test_gst_gpu import read_records
from tests.util import cut_clip, frames, pad_planes

pytestmark = pytest.mark.gpu

NZ_T8 = 1 << 27


def _clip(kind, w, h, n):
    if kind == "s2":
        return [f[:2] for f in frames(w, h, n)]
    return [pad_planes(y, uv) for y, uv in synth.s4_frames(w, h, n)]


def _field(oracle, cy, ry, qp, iters=3):
    surf, imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
    for _ in range(iters):
        imv = oracle.me_select(surf, imv, cy.shape[1] // 16, cy.shape[0] // 16, 16, qp, threads=8)
    return surf, imv


def _mb_out(res, n, mbw):
    """record, levels, luma and chroma reconstruction of macroblock n"""
    rec_y, rec_uv, mbi, lev = res
    mby, mbx = divmod(n, mbw)
    return (mbi[n].tobytes(), lev[n].tobytes(), rec_y[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16].tobytes(),
            rec_uv[8 * mby:8 * mby + 8, 16 * mbx:16 * mbx + 16].tobytes())


CASES = [(k, w, h, qp, drop) for k in ("s2", "s4") for (w, h) in ((176, 144), (640, 368)) for qp in (22, 30, 38) for drop in (0, 4)]
CASES += [(k, 1920, 1088, qp, 0) for k in ("s2", "s4") for qp in (22, 38)] + [("s4", 1920, 1088, 30, 4)]


@pytest.mark.parametrize("kind,w,h,qp,drop", CASES)
def test_adaptive_stage_is_the_splice_of_the_fixed_ones(E, oracle, kind, w, h, qp, drop):
    """stage_pmb on three handles, transform8x8 = 0, 1, 2, from the same oracle field, surfaces and intra decisions, macroblocks independent (no intra
    pass): every macroblock of the adaptive picture -- record, levels, reconstruction before deblocking -- is the 8x8 handle's where t8ref.decide()
    on the device's final vector chooses 8x8, else the 4x4 handle's.  Modes 0 and 1 are oracle-exact (test_parity_gpu.py), so this pins mode 2 to
    the oracle through the rule."""
    clip = _clip(kind, w, h, 2)
    (cy, cuv), (ry, ruv) = clip[1], clip[0]
    mbh, mbw = h // 16, w // 16
    surf, imv = _field(oracle, cy, ry, qp)
    idec = oracle.intra_decide(oracle.intra_analyse(cy, cuv), mbw, mbh, qp, False)
    res = {}
    for mode in (0, 1, 2):
        e = E.Encoder(w, h, fixed_qp=qp, transform8x8=mode)
        res[mode] = e.stage_pmb(cy, cuv, ry, ruv, imv, oracle.surf_to_device(surf), qp, drop=drop, refine=True, idec=idec, run_intra_p=False)
        e.close()
    m0, m1, m2 = res[0][2], res[1][2], res[2][2]
    for f in ("mvx", "mvy", "mb_type", "i16_mode", "chroma_mode", "qp", "cost"):
        assert np.array_equal(m2[f], m0[f]) and np.array_equal(m2[f], m1[f]), f
    n8 = n4 = 0
    for n in range(mbw * mbh):
        o0, o1, o2 = _mb_out(res[0], n, mbw), _mb_out(res[1], n, mbw), _mb_out(res[2], n, mbw)
        if o0 == o1:  # not coded with a luma residual that the transform size changes: nothing to choose
            assert o2 == o0, n
            continue
        mby, mbx = divmod(n, mbw)
        use8 = t8ref.decide(cy, ry, mbx, mby, int(m2["mvx"][n]), int(m2["mvy"][n]))
        want = o1 if use8 else o0
        assert o2 == want, (n, use8, [a == b for a, b in zip(o2, want)])
        n8 += use8
        n4 += not use8
    if drop == 0 and qp <= 30:
        assert n8 > 0 and n4 > 0, (n8, n4)  # both kinds of coded macroblock
    t8 = (m2["nzmask"] & NZ_T8) != 0
    assert not (t8 & ((m2["nzmask"] & 0xFFFF) == 0)).any()  # transform_size_8x8_flag only with luma levels


def _sps_profile(au):
    i = au.find(b"\x00\x00\x01")
    while i >= 0:
        if au[i + 3] & 31 == 7:
            return au[i + 4]
        i = au.find(b"\x00\x00\x01", i + 3)
    return None


STREAMS = [  # w, h, n, depth, exclusive, i8x8, aq, intra_in_p
    (322, 182, 6, 0, False, True, False, 1),
    (322, 182, 6, 2, True, False, True, 2),
    (640, 368, 6, 0, True, True, True, 2),
    (640, 368, 6, 2, False, False, False, 1),
    (1280, 720, 5, 0, False, False, True, 1),
    (1280, 720, 5, 2, True, True, False, 2),
    (1920, 1080, 4, 0, True, True, False, 2),
    (1920, 1080, 4, 2, False, True, True, 1),
]


@pytest.mark.parametrize("w,h,n,depth,exclusive,i8,aq,iip", STREAMS)
def test_adaptive_streams_decode_to_the_recon(E, oracle, w, h, n, depth, exclusive, i8, aq, iip):
    """Encoder(transform8x8=2) with the library's slicing: every access unit decodes (independent decoder) to the device's reconstruction (per picture at
    depth 0, the last one at depth 2); without adaptive quantisation the oracle's deblocking of the device's picture before the filter, with the stream's
    slice settings, is its reconstruction; the SPS says High; P pictures hold coded inter macroblocks with and without the 8x8 transform."""
    clip = cut_clip(w, h, n, 3)
    qps = [30, 26, 34, 22]
    e = E.Encoder(w, h, gop=30, fixed_qp=30, transform8x8=2, keep_prefilter=True, pipeline_depth=depth, exclusive=exclusive, i8x8=i8, aq=aq,
                  intra_in_p=iip, slices=None, slice_deblock=None)
    dec = oracle.Decoder()
    oracle.set_transform8x8(True)
    kinds = np.zeros(2, np.int64)
    try:
        got = []
        for i, (y, uv) in enumerate(clip):
            e.set_fixed_qp(qps[i % len(qps)])
            if depth == 0:
                au, key = e.encode(y, uv, pts=i)
                if i == 0:
                    assert key and _sps_profile(au) == 100
                dy, duv = dec.decode(au)
                ry, ruv = e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)
                assert np.array_equal(dy, ry[:dy.shape[0], :dy.shape[1]]) and np.array_equal(duv, ruv[:duv.shape[0], :duv.shape[1]]), i
                mbi = e.fetch(E.FETCH_MBINFO)
                if not aq:
                    rows = e.slice_rows if key else e.p_slice_rows
                    oracle.set_slice_rows(rows)
                    oracle.set_slice_deblock(2 if rows else 0)
                    want_y, want_uv = oracle.deblock_frame(e.fetch(E.FETCH_PREFILTER_Y), e.fetch(E.FETCH_PREFILTER_UV), mbi)
                    assert np.array_equal(want_y, ry) and np.array_equal(want_uv, ruv), i
                if not key:
                    coded = (mbi["mb_type"] == 1) & ((mbi["nzmask"] & 0xFFFF) != 0)
                    t8 = (mbi["nzmask"] & NZ_T8) != 0
                    kinds += [(coded & t8).sum(), (coded & ~t8).sum()]
            else:
                e.submit(y, uv, pts=i)
                if e.pending > depth:
                    got.append(e.collect()[0])
        if depth:
            while e.pending:
                got.append(e.collect()[0])
            assert _sps_profile(got[0]) == 100
            for au in got:
                dy, duv = dec.decode(au)
            ry, ruv = e.fetch(E.FETCH_RECON_Y), e.fetch(E.FETCH_RECON_UV)
            assert np.array_equal(dy, ry[:dy.shape[0], :dy.shape[1]]) and np.array_equal(duv, ruv[:duv.shape[0], :duv.shape[1]])
        else:
            assert kinds[0] > 0 and kinds[1] > 0, kinds
    finally:
        oracle.set_transform8x8(False)
        oracle.set_slice_rows(0)
        oracle.set_slice_deblock(0)
        dec.close()
        e.close()


def _stream(E, clip, w, h, **kw):
    e = E.Encoder(w, h, gop=30, fixed_qp=30, transform8x8=2, **kw)
    depth = kw.get("pipeline_depth", 0)
    out = []
    for i, (y, uv) in enumerate(clip):
        e.set_fixed_qp([30, 24, 36][i % 3])
        e.submit(y, uv, pts=i)
        if e.pending > depth:
            out.append(e.collect()[0])
    while e.pending:
        out.append(e.collect()[0])
    e.close()
    return out


@pytest.mark.parametrize("depth", [0, 2])
def test_adaptive_stream_does_not_depend_on_the_schedule(E, depth):
    """Byte-identical streams with exclusive on and off, graphs on and off, either deblocking form, one HIP stream, and twice over."""
    w, h = 640, 368
    clip = cut_clip(w, h, 6, 3)
    base = _stream(E, clip, w, h, pipeline_depth=depth)
    assert base == _stream(E, clip, w, h, pipeline_depth=depth)
    for kw in (dict(exclusive=True), dict(use_graphs=False), dict(deblock_mode=1), dict(single_stream=True)):
        assert _stream(E, clip, w, h, pipeline_depth=depth, **kw) == base, kw


def test_two_kernel_stage_refuses_the_adaptive_mode(E, oracle):
    """mi355enc_stage_inter has no per-macroblock choice: a transform8x8 = 2 handle gets MI355ENC_ERR_ARG, a transform8x8 = 1 handle runs."""
    (cy, cuv), (ry, ruv) = [f[:2] for f in frames(64, 48, 2)][::-1]
    mbi = oracle.imv_to_mbinfo(_field(oracle, cy, ry, 30)[1], 30)
    e = E.Encoder(64, 48, fixed_qp=30, transform8x8=2)
    L = e.L
    rec_y, rec_uv = np.empty_like(cy), np.empty_like(cuv)
    lev = np.empty((mbi.size, E.LEVELS_PER_MB), np.int16)
    m = mbi.copy()
    p = lambda a: a.ctypes.data_as(E.C.c_void_p)
    assert L.mi355enc_stage_inter(e.h, p(cy), p(cuv), p(ry), p(ruv), 30, p(m), p(rec_y), p(rec_uv), p(lev)) == E.ERR_ARG
    e.close()
    e = E.Encoder(64, 48, fixed_qp=30, transform8x8=1)
    e.stage_inter(cy, cuv, ry, ruv, mbi, 30)
    e.close()


@pytest.mark.skipif(not os.path.exists(HARNESS), reason="oracle/_ref/ref_harness not shipped")
def test_dct8x8_adaptive_property_gives_a_high_profile_stream_that_decodes(tmp_path, oracle):
    """`dct8x8=true dct8x8-adaptive=true`: a High-profile stream the independent decoder takes, whose P pictures differ from the forced 8x8 transform's."""
    streams = {}
    for adaptive in ("false", "true"):
        pf = tmp_path / ("pipe_" + adaptive)
        pf.write_text("videotestsrc num-buffers=8 pattern=zone-plate kx2=12 ky2=12 kt=2 ! video/x-raw,width=640,height=368,framerate=30/1,format=NV12 ! "
                      "mi355h264enc key-int-max=4 qp=28 dct8x8=true dct8x8-adaptive=%s name=venc_bps ! appsink name=appsink sync=false\n" % adaptive)
        out = tmp_path / ("out_%s.bin" % adaptive)
        r = subprocess.run([HARNESS, str(pf), str(out)], env=gst_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        recs = read_records(str(out))
        assert len(recs) == 8
        assert recs[0][1][:5] == b"\x00\x00\x00\x01\x67" and recs[0][1][5] == 100  # profile_idc of the SPS: High
        dec = oracle.Decoder()
        for _, au in recs:
            dec.decode(au)
        assert dec.size == (640, 368)
        streams[adaptive] = [au for _, au in recs]
    assert streams["true"][0] == streams["false"][0]  # I pictures do not change
    assert streams["true"][1:4] != streams["false"][1:4]
