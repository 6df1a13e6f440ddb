"""What tests/test_extremes_cpu.py and tests/test_extremes_gpu.py share: the geometries, QPs, seeds and inputs at the arithmetic limits, so
that the conditions asserted on the oracle alone (CPU) are conditions on exactly the inputs the kernels are run on (GPU)."""
import contextlib
import functools

import numpy as np

from tests.util import near_sat_ramps, pad_planes, sat_blocks, sat_clip, shifted_pair, stripes

GEOMS = [(16, 16), (64, 48), (50, 34), (176, 144)]  # one macroblock; interior macroblocks and every edge; an odd size; more than one strip of the search
QPS = [0, 5, 6, 30, 51]                             # 5 -> 6: the qbits step; 51: the largest lambda
BLKS = [16, 8, 4, 1]
PERIODS = [2, 3, 4, 6]
AXES = ["v", "h", "both"]
SHIFTS = [(16, 16), (-16, -16), (16, -16), (-16, 16)]
SEED_CUR, SEED_REF, SEED_SHIFT, SEED_RAMPS, SEED_DB, SEED_REC, SEED_CLIP = 8, 108, 21, 31, 41, 42, 51

STREAM_GEOMS = [(64, 48), (176, 144)]
STREAM_QPS = [0, 51, 3, 26, 6, 40]
STREAM_GOP, STREAM_N = 3, 6


def max_au_bytes(w, h):
    """mi355enc_max_au_bytes of an encoder of this size (h264_host.c, h264_max_au_bytes); the GPU tests check that the library says the same"""
    return ((w + 15) // 16) * ((h + 15) // 16) * 1536 + 4096


def _padded(p):
    return pad_planes(*p)


@functools.lru_cache(maxsize=None)
def sat_pair(w, h, blk):
    """-> ((cur_y, cur_uv), (ref_y, ref_uv)) at the coded size: two independent sat_blocks pictures"""
    return _padded(sat_blocks(w, h, blk, SEED_CUR)), _padded(sat_blocks(w, h, blk, SEED_REF))


@functools.lru_cache(maxsize=None)
def stripes_pair(w, h, period, axis):
    """The reference is the stripes; the current picture is the rounded average of the stripes and the stripes moved by one sample -- the
    picture half a sample along, so that the refinement has a fractional position to find (period 2 "both": flat grey, every position ties)."""
    a, b = stripes(w, h, period, axis, 0), stripes(w, h, period, axis, 1)
    cur = tuple(((p.astype(np.int32) + q + 1) >> 1).astype(np.uint8) for p, q in zip(a, b))
    return _padded(cur), _padded(a)


@functools.lru_cache(maxsize=None)
def shifted(w, h, dx, dy, half=False):
    cur, ref = shifted_pair(w, h, dx, dy, SEED_SHIFT, half)
    return _padded(cur), _padded(ref)


@functools.lru_cache(maxsize=None)
def ramps(w, h):
    return _padded(near_sat_ramps(w, h, SEED_RAMPS))


@functools.lru_cache(maxsize=None)
def pair(kind, w, h):
    """The picture pairs by name: ("sat", blk), ("stripes", period, axis), ("shift", dx, dy, half)"""
    return {"sat": sat_pair, "stripes": stripes_pair, "shift": shifted}[kind[0]](w, h, *kind[1:])


SAT_KINDS = [("sat", b) for b in BLKS]
STRIPE_KINDS = [("stripes", p, a) for p in PERIODS for a in AXES]
SHIFT_KINDS = [("shift", dx, dy, False) for dx, dy in SHIFTS] + [("shift", dx, dy, True) for dx, dy in SHIFTS]

_fields = {}


def settled_field(oracle, kind, w, h, qp, iters=3):
    """(surfaces, field after `iters` selection passes) of a named pair on the oracle, computed once"""
    key = (kind, w, h, qp, iters)
    if key not in _fields:
        (cy, _), (ry, _) = pair(kind, w, h)
        surf, imv = oracle.me_frame(cy, ry, 16, qp, threads=8)
        for _ in range(iters):
            imv = oracle.me_select(surf, imv, cy.shape[1] // 16, cy.shape[0] // 16, 16, qp, threads=8)
        _fields[key] = (surf, imv)
    return _fields[key]


@contextlib.contextmanager
def oracle_mode(oracle, t8=False, i8=False, part=False, i4=True, slice_rows=0):
    """the oracle's process-wide switches, put back afterwards"""
    oracle.set_transform8x8(t8)
    oracle.set_i8x8(i8)
    oracle.set_i4x4(i4)
    oracle.set_slice_rows(slice_rows)
    oracle.set_features(oracle.F_ALL | (oracle.F_PART if part else 0))
    try:
        yield
    finally:
        oracle.set_transform8x8(False)
        oracle.set_i8x8(False)
        oracle.set_i4x4(True)
        oracle.set_slice_rows(0)
        oracle.set_features(oracle.F_ALL)


# name -> (ceracoder_amd.enc.Encoder arguments, oracle_mode arguments, oracle.Encoder arguments; "lib": the library's default configuration)
STREAM_CFGS = {
    "baseline": ({}, {}, {}),
    "preset2": (dict(transform8x8=True, i8x8=True, aq=True), dict(t8=True, i8=True), dict(aq=True)),
    "partitions": (dict(partitions=True), dict(part=True), {}),
    "lib": (dict(slices=None, slice_deblock=None), {}, "lib"),
    "depth0": (dict(pipeline_depth=0, exclusive=True), {}, {}),
    "depth2": (dict(pipeline_depth=2, exclusive=True), {}, {}),
}


@functools.lru_cache(maxsize=None)
def stream_clip(w, h):
    return sat_clip(w, h, STREAM_N, SEED_CLIP)


_streams = {}


def oracle_stream(oracle, w, h, cfg):
    """[(access unit, is key, recon_y, recon_uv, records, levels)] of the sat_clip stream under a configuration, from the oracle (computed once)"""
    _, mode, okw = STREAM_CFGS[cfg]
    if okw == "lib":
        okw = dict(intra_slices=0, p_slices=oracle.auto_slices((h + 15) // 16), slice_deblock_local=True)
    key = (w, h, tuple(sorted(mode.items())), tuple(sorted(okw.items())))
    if key not in _streams:
        out = []
        with oracle_mode(oracle, **mode):
            oe = oracle.Encoder(w, h, gop=STREAM_GOP, threads=8, scenecut=False, **okw)
            for i, (y, uv) in enumerate(stream_clip(w, h)):
                au, is_key = oe.encode(y, uv, STREAM_QPS[i % len(STREAM_QPS)])
                out.append((au, is_key, oe.recon_y, oe.recon_uv, oe.mbinfo, oe.levels))
            oe.close()
        _streams[key] = out
    return _streams[key]
