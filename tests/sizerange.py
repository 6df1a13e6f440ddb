"""What tests/test_size_range_cpu.py and tests/test_size_range_gpu.py share: the geometries at the ends of the accepted size range (16 .. 8192 per axis), the
clips, QPs and toolsets, so that the conditions asserted on the oracle alone (CPU) are conditions on exactly the inputs the kernels are run on (GPU)."""
import functools

import numpy as np

from ceracoder_amd import synth
from tests import extremes as X
from tests.util import pad_planes

# mbw 512: the last word of the intra rows' bit sets; 8190 x 34: visible size 2 short of the coded size; 4112: mbw 257, the first width past what had run;
# 8176: mbw 511; 8192 x 144: nine rows -- three deblocking bands, the last of one row -- and 4608 macroblocks
WIDE = [(8192, 16), (8192, 48), (8190, 34), (4112, 32), (8176, 32), (8192, 144)]
TALL = [(16, 8192), (48, 8192), (34, 8190), (32, 4112), (144, 8192)]
STRIPS = WIDE + TALL

STRIP_QP = 30                                     # the fixed QP of the stage tests and of the conditions
STREAM_N, STREAM_GOP = 5, 3
PMB_POINTS = [(30, 0), (51, 8), (0, 0)]           # (qp, drop) of the fused P stage
REFRESH_STRIPS = [(8192, 48), (48, 8192)]

GRID = range(1, 10)                               # mbw and mbh of the remainder sweep
GRID_N, GRID_QP = 4, 28

# (w, h): nmb at the last size of a levels_scan_kernel instantiation and at the first of the next (k_handover.hip: 4096 / 8192 / 32768)
THRESHOLDS = [(1024, 1024), (1040, 1024), (2048, 1024), (2064, 1024), (4096, 2048), (4112, 2048)]
THRESHOLD_QP = 32

INPUT_SHAPES = [(8192, 16), (8190, 18), (16, 8192), (18, 8190)]


def is_wide(w, h):
    return w >= h


def mb_size(w, h):
    return (w + 15) // 16, (h + 15) // 16


WAIT_WGS_MAX = 192   # an MI355X has 256 compute units; a quarter stays free of workgroups that wait for another kernel (enc_handle.cpp: wait_room)


def wait_wgs(mbw, mbh):
    """workgroups of a P picture's band-deblocking launch with three pictures in flight (mi355enc_dev.h, db_launch_wgs): two per band of four rows, four where
    the bands are walked in two parts (mbw >= 60), and one per macroblock row where the intra rows ride in the launch (up to 3600 macroblocks)"""
    return (4 if mbw >= 60 else 2) * ((mbh + 3) // 4) + (mbh if mbw * mbh <= 3600 else 0)


def grid_size(mbw, mbh):
    """visible size 2 short of the coded size wherever it can be"""
    return max(16, 16 * mbw - 2), max(16, 16 * mbh - 2)


def grid_cells(kind):
    """(mbw, mbh) of the sweep: "full", or "frame": the diagonal plus the first and last row and column"""
    if kind == "full":
        return [(a, b) for b in GRID for a in GRID]
    return [(a, b) for b in GRID for a in GRID if a == b or a in (1, 9) or b in (1, 9)]


@functools.lru_cache(maxsize=None)
def strip_clip(w, h, n=STREAM_N):
    """The S2 clip with two flat patches per picture i, luma 40 + 37 i and both chroma components 100 + 20 i: over the last 200 columns (rows of a tall strip)
    and over the 48 around the middle.  A flat patch that changes level is cheaper intra than inter, so the P pictures carry intra macroblocks in the last
    column and around mbw / 2 (where the band deblocker looks for its cut), which S2 alone does not give beyond column 480."""
    out = []
    for i, (y, uv) in enumerate(synth.s2_frames(w, h, n)):
        y, uv = y.copy(), uv.copy()
        ext = w if is_wide(w, h) else h
        for lo, hi in ((max(0, ext - 200), ext), (max(0, ext // 2 - 24), ext // 2 + 24)):
            if is_wide(w, h):
                y[:, lo:hi], uv[:, lo:hi] = 40 + 37 * i, 100 + 20 * i
            else:
                y[lo:hi], uv[lo // 2:hi // 2] = 40 + 37 * i, 100 + 20 * i
        out.append((y, uv))
    return out


@functools.lru_cache(maxsize=None)
def strip_pair(w, h):
    """((cur_y, cur_uv), (ref_y, ref_uv)) at the coded size: picture 1 against picture 0 of strip_clip"""
    c = strip_clip(w, h)
    return pad_planes(*c[1]), pad_planes(*c[0])


@functools.lru_cache(maxsize=None)
def grid_clip(w, h):
    return [(y, uv) for y, uv in synth.s2_frames(w, h, GRID_N)]


@functools.lru_cache(maxsize=None)
def threshold_clip(w, h):
    return [(y, uv) for y, uv in synth.s2_frames(w, h, 2)]


_fields, _streams = {}, {}


def settled_field(oracle, w, h, qp, iters=3):
    """(surfaces, [first selection, pass 1, .. pass iters]) of strip_pair on the oracle, computed once"""
    key = (w, h, qp, iters)
    if key not in _fields:
        (cy, _), (ry, _) = strip_pair(w, h)
        surf, imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
        fields = [imv]
        for _ in range(iters):
            fields.append(oracle.me_select(surf, fields[-1], cy.shape[1] // 16, cy.shape[0] // 16, 16, qp, threads=8))
        _fields[key] = (surf, fields)
    return _fields[key]


# name -> (ceracoder_amd.enc.Encoder arguments, oracle_mode arguments, oracle.Encoder arguments or a function of (oracle, mbh) giving them)
def _lib_okw(oracle, mbh):
    return dict(intra_slices=0, p_slices=oracle.auto_slices(mbh), slice_deblock_local=True)


def _aq_sliced(oracle, mbh):
    return dict(aq=True, intra_slices=min(3, mbh), p_slices=min(3, mbh), slice_deblock_local=False)


STREAM_CFGS = {k: (v[0], v[1], _lib_okw if v[2] == "lib" else v[2]) for k, v in X.STREAM_CFGS.items()}
STREAM_CFGS["i4-in-p"] = (dict(intra_in_p=2), dict(i4p=True), {})
STREAM_CFGS["aq-sliced"] = (None, {}, _aq_sliced)   # the library's arguments depend on mbh: enc_args()
GRID_CFGS = {
    "baseline-depth0": (dict(pipeline_depth=0, exclusive=True), {}, {}),
    "lib-depth2": (dict(slices=None, slice_deblock=None, pipeline_depth=2, exclusive=True), {}, _lib_okw),
    "preset2-aq": (dict(transform8x8=True, i8x8=True, aq=True), dict(t8=True, i8=True), dict(aq=True)),
}
THRESHOLD_CFGS = {"plain": ({}, {}, {}), "aq": (dict(aq=True), {}, dict(aq=True))}


def enc_args(cfgs, cfg, h):
    """ceracoder_amd.enc.Encoder arguments of a configuration at a height"""
    kw = cfgs[cfg][0]
    if kw is None:  # aq-sliced: three slices in I and P pictures (one per row where there are no more rows), so that the QP_Y chain starts again with every slice
        s = min(3, (h + 15) // 16)
        kw = dict(aq=True, intra_slices=s, slices=s, slice_deblock=False)
    return kw


def oracle_stream(oracle, cfgs, cfg, w, h, clip, qps, gop, name="strip"):
    """[(access unit, is key, recon_y, recon_uv, records)] of a clip under a configuration, from the oracle (computed once); every access unit went through the
    independent decoder, whose output is asserted equal to the reconstruction here"""
    _, mode, okw = cfgs[cfg]
    if callable(okw):
        okw = okw(oracle, (h + 15) // 16)
    key = (name, w, h, gop, tuple(qps), len(clip), tuple(sorted(mode.items())), tuple(sorted(okw.items())))  # (toolsets that differ only in the library's schedule share a stream)
    if key not in _streams:
        mode = dict(mode)
        i4p = mode.pop("i4p", False)
        out = []
        with X.oracle_mode(oracle, **mode):
            if i4p:
                oracle.set_features(oracle.F_ALL | oracle.F_I4P)
            try:
                oe = oracle.Encoder(w, h, gop=gop, threads=8, scenecut=False, **okw)
                dec = oracle.Decoder()
                for i, (y, uv) in enumerate(clip):
                    au, is_key = oe.encode(y, uv, qps[i % len(qps)])
                    ry, ruv = oe.recon_y, oe.recon_uv
                    dy, duv = dec.decode(au)
                    assert np.array_equal(dy, ry) and np.array_equal(duv, ruv), ("the oracle's decoder differs from its encoder", cfg, w, h, i)
                    out.append((au, is_key, ry, ruv, oe.mbinfo))
                assert dec.size == (w, h)
                oe.close(); dec.close()
            finally:
                oracle.set_features(oracle.F_ALL)
        _streams[key] = out
    return _streams[key]


def strip_stream(oracle, cfg, w, h):
    return oracle_stream(oracle, STREAM_CFGS, cfg, w, h, strip_clip(w, h), X.STREAM_QPS, STREAM_GOP)


def fixed_qp_stream(oracle, w, h, n=4):
    """the first n pictures of strip_clip at STRIP_QP, one IDR picture and P pictures: what the CPU conditions are asserted on"""
    return oracle_stream(oracle, STREAM_CFGS, "baseline", w, h, strip_clip(w, h)[:n], [STRIP_QP], 60)


def grid_stream(oracle, cfg, mbw, mbh):
    w, h = grid_size(mbw, mbh)
    return oracle_stream(oracle, GRID_CFGS, cfg, w, h, grid_clip(w, h), [GRID_QP], 60, "grid")


def threshold_stream(oracle, cfg, w, h):
    return oracle_stream(oracle, THRESHOLD_CFGS, cfg, w, h, threshold_clip(w, h), [THRESHOLD_QP], 60, "threshold")
