"""Periodic intra refresh on the device (mi355enc_set_intra_refresh): whole streams through the independent decoder against
the device's reconstruction, the stream's structure against tests/irref.py, a decoder that joins mid-stream with a garbage reference, the setter's
refusals, and CBR under the committed balancer script."""
import os

import numpy as np
import pytest

from ceracoder_amd import enc as E_
from ceracoder_amd import synth
from tests import irref
from tests.spsref import slice_frame_num as _frame_num

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clip(w, h, n):
    return list(synth.s2_frames(w, h, n))


def _pic(clip, i):
    k = i % (2 * len(clip) - 2)
    return clip[k if k < len(clip) else 2 * len(clip) - 2 - k]


def _encode(e, clip, n, depth, force=(), skip=(), fetch=False):
    """n pictures; force: indices submitted as forced key units; skip: indices submitted with set_fixed_drop(DROP_SKIP).  Returns the access
    units, their keyframe flags and drop levels, and (fetch) the device's reconstruction of every picture (depth 0) or of the last one."""
    aus, keys, drops, recs = [], [], [], []

    def take():
        au, key, _, _ = e.collect()
        aus.append(au); keys.append(key); drops.append(e.last_drop)
        if fetch and depth == 0:
            recs.append((e.fetch(E_.FETCH_RECON_Y), e.fetch(E_.FETCH_RECON_UV)))

    for i in range(n):
        if skip:
            e.set_fixed_drop(irref.DROP_SKIP if i in skip else 0)
        y, uv = _pic(clip, i)
        e.submit(y, uv, pts=i, force_idr=i in force)
        while e.pending > depth:
            take()
    while e.pending:
        take()
    if fetch and depth:
        recs.append((e.fetch(E_.FETCH_RECON_Y), e.fetch(E_.FETCH_RECON_UV)))
    return aus, keys, drops, recs


def _nals(au):
    out, i = [], au.find(b"\x00\x00\x01")
    while i >= 0:
        j = au.find(b"\x00\x00\x01", i + 3)
        body = au[i + 3:j if j >= 0 else len(au)].rstrip(b"\x00")
        out.append((body[0] & 31, body[1:]))
        i = j
    return out


def _sei_recovery(payload):
    """payloadType, payloadSize, recovery_frame_cnt, exact_match_flag, broken_link_flag, changing_slice_group_idc of an SEI NAL's first message"""
    rb = payload.replace(b"\x00\x00\x03", b"\x00\x00")
    ptype, size = rb[0], rb[1]
    bits = "".join("{:08b}".format(b) for b in rb[2:2 + size])
    z = bits.index("1")
    cnt = int(bits[z:2 * z + 1], 2) - 1
    p = 2 * z + 1
    return ptype, size, cnt, int(bits[p]), int(bits[p + 1]), int(bits[p + 2:p + 4], 2)


def _open(E, w, h, n, qp=28, depth=0, slices=None, iip=1, t8=0, aq=False, on=True, gop=None):
    kw = dict(slices=None, slice_deblock=None) if slices is None else dict(slices=slices)
    return E.Encoder(w, h, fps=60, gop=gop or n, fixed_qp=qp, pipeline_depth=depth, exclusive=depth == 2, intra_in_p=iip, transform8x8=t8, aq=aq,
                     scenecut=False, intra_refresh=on, **kw)


def _check_structure(aus, keys, drops, wants, mbw, mbh, n, oracle, recs, depth):
    """decode everything; check keyframes, NAL layout, forced columns, vectors and Intra_4x4 modes against irref; returns the decoded pictures"""
    pics = irref.schedule(mbw, n, wants)
    dec = oracle.Decoder()
    mbi, lev = dec.capture(mbw * mbh)
    out = []
    for i, (au, key, pic) in enumerate(zip(aus, keys, pics)):
        y, uv = dec.decode(au)
        out.append((y, uv))
        types = [t for t, _ in _nals(au)]
        assert (drops[i] == irref.DROP_SKIP) == (pic["kind"] == "skip"), (i, drops[i], pic)
        if pic["kind"] == "idr":
            assert types[:2] == [7, 8] and 5 in types and key, (i, types)
            continue
        assert 5 not in types, (i, types)
        assert key == pic["start"], (i, key, pic)
        if pic["start"]:
            assert types[:3] == [7, 8, 6] and set(types[3:]) == {1}, (i, types)
            ptype, _, cnt, exact, broken, csg = _sei_recovery(_nals(au)[2][1])
            assert (ptype, cnt, exact, broken, csg) == (6, n - 1, 1, 0, 0), i
        else:
            assert set(types) == {1}, (i, types)
        if pic["kind"] == "skip":
            continue
        g = mbi.reshape(mbh, mbw)
        assert (g["mb_type"][:, pic["c0"]:pic["c1"]] != 1).all(), (i, pic)          # the refresh columns are intra
        inter = g["mb_type"] == 1
        for mx in range(pic["c0"]):
            for v in np.unique(g["mvx"][:, mx][inter[:, mx]]):
                assert irref.vector_ok(mx, int(v), pic), (i, mx, int(v), pic)
        if pic["c1"] < mbw and pic["c1"] > 0:
            col = lev.reshape(mbh, mbw, -1)[:, pic["c1"] - 1, 256 + 5]
            i4 = g["mb_type"][:, pic["c1"] - 1] == 2
            assert all(irref.i4_mode_ok(pic, pic["c1"] - 1, mbw, 5, int(m)) for m in col[i4]), (i, pic)
    if depth == 0:
        for i, ((y, uv), (ry, ruv)) in enumerate(zip(out, recs)):
            assert np.array_equal(y, ry) and np.array_equal(uv, ruv), i
    else:
        assert np.array_equal(out[-1][0], recs[-1][0]) and np.array_equal(out[-1][1], recs[-1][1])
    dec.close()
    return out, pics


CFGS = [  # w, h, slices, intra_in_p, transform8x8, aq, pipeline_depth
    (1920, 1080, None, 1, 0, False, 0),
    (1920, 1080, 1, 2, 2, True, 2),
    (1920, 1080, None, 2, 1, False, 2),
    (1280, 720, None, 2, 1, True, 0),
    (1280, 720, 1, 1, 2, False, 2),
    (176, 144, None, 2, 0, True, 2),
    (176, 144, 1, 1, 1, False, 0),
    (176, 144, None, 2, 2, False, 0),
]


@pytest.mark.parametrize("w,h,slices,iip,t8,aq,depth", CFGS)
def test_stream_decodes_to_the_reconstruction_and_follows_the_schedule(E, oracle, w, h, slices, iip, t8, aq, depth):
    n = 8
    npic = 1 + 2 * n + 3
    e = _open(E, w, h, n, depth=depth, slices=slices, iip=iip, t8=t8, aq=aq)
    aus, keys, drops, recs = _encode(e, _clip(w, h, 12), npic, depth, fetch=True)
    mbw, mbh = e.mbw, e.mbh
    e.close()
    _check_structure(aus, keys, drops, ["idr"] + ["p"] * (npic - 1), mbw, mbh, n, oracle, recs, depth)


def _join(oracle, aus, k, mbw, mbh, seed=7):
    """decode AU 0, overwrite the reference with noise, decode from AU k on"""
    dec = oracle.Decoder()
    dec.decode(aus[0])
    g = np.random.default_rng(seed)
    oracle._view(dec.L.orc_dec_y(dec.h), (16 * mbh, 16 * mbw), np.uint8)[:] = g.integers(0, 256, (16 * mbh, 16 * mbw), dtype=np.uint8)
    oracle._view(dec.L.orc_dec_uv(dec.h), (8 * mbh, 16 * mbw), np.uint8)[:] = g.integers(0, 256, (8 * mbh, 16 * mbw), dtype=np.uint8)
    out = [dec.decode(au) for au in aus[k:]]
    dec.close()
    return out


@pytest.mark.parametrize("w,h,depth", [(1280, 720, 0), (1920, 1080, 2)])
def test_a_decoder_joining_at_a_cycle_start_converges(E, oracle, w, h, depth):
    """The stream: IDR, three cycles, a forced key unit, two more cycles, with one all-skip picture in the middle of the third cycle and one wanted
    for the last picture of the fifth (it moves to the next cycle's first picture).  A decoder that starts at a cycle's first picture with a noise
    reference outputs picture k + N - 1 and every later one bit-exactly, and the clean columns of each earlier picture already."""
    n = 6
    force = {1 + 3 * n + 2}
    skip = {1 + 2 * n + 2, 1 + 3 * n + 3 + 2 * n - 1}
    npic = 1 + 3 * n + 3 + 2 * n + 3
    wants = ["idr" if i == 0 or i in force else "skip" if i in skip else "p" for i in range(npic)]
    e = _open(E, w, h, n, depth=depth, iip=2, t8=2)
    aus, keys, drops, recs = _encode(e, _clip(w, h, 12), npic, depth, force=force, skip=skip, fetch=True)
    mbw, mbh = e.mbw, e.mbh
    e.close()
    full, pics = _check_structure(aus, keys, drops, wants, mbw, mbh, n, oracle, recs, depth)
    starts = [i for i, p in enumerate(pics) if p["start"]]
    moved = max(skip)
    assert pics[moved]["kind"] == "p" and pics[moved + 1]["kind"] == "skip" and pics[moved + 1]["start"]  # (the all-skip picture moved to the next cycle)
    first, later, after_idr = starts[0], starts[2], [s for s in starts if s > min(force)][0]
    for k in (first, later, after_idr):
        joined = _join(oracle, aus, k, mbw, mbh)
        for i, (y, uv) in enumerate(joined):
            fy, fuv = full[k + i]
            if i >= n - 1:
                assert np.array_equal(y, fy) and np.array_equal(uv, fuv), (k, i)
            else:
                ly, lc = irref.exact_cols(pics[k + i], mbw)
                assert np.array_equal(y[:, :ly], fy[:, :ly]) and np.array_equal(uv[:, :2 * lc], fuv[:, :2 * lc]), (k, i, ly, lc)
        assert not np.array_equal(joined[0][0], full[k][0])  # (the noise did reach the picture)


def test_without_refresh_a_joining_decoder_does_not_converge(E, oracle):
    """Control: the same join on a stream with refresh off and no IDR picture in the window stays wrong."""
    w, h, n = 1280, 720, 6
    e = _open(E, w, h, n, on=False, gop=1000, iip=2)
    aus, _, _, _ = _encode(e, _clip(w, h, 12), 1 + 3 * n, 0)
    mbw, mbh = e.mbw, e.mbh
    e.close()
    dec = oracle.Decoder()
    full = [dec.decode(au) for au in aus]
    dec.close()
    joined = _join(oracle, aus, 1, mbw, mbh)
    assert not np.array_equal(joined[-1][0], full[-1][0])


def test_setter_refusals(E):
    e = E.Encoder(176, 144, gop=8, fixed_qp=30)
    e.set_intra_refresh(True)
    e.set_intra_refresh(False)
    e.set_intra_refresh(True)
    y, uv = _clip(176, 144, 1)[0]
    e.submit(y, uv)
    with pytest.raises(E.EncoderError):
        e.set_intra_refresh(False)                     # after the first submit
    e.collect()
    e.close()
    for kw in (dict(intra_in_p=0), dict(partitions=True), dict(gop=1), dict(gop=257), dict(gop=100000)):
        args = dict(gop=8, fixed_qp=30)
        args.update(kw)
        e = E.Encoder(176, 144, **args)
        with pytest.raises(E.EncoderError):
            e.set_intra_refresh(True)
        e.set_intra_refresh(False)                     # (off is always accepted before the first submit)
        e.close()
    e = E.Encoder(176, 144, gop=256, fixed_qp=30)      # the longest period whose recovery_frame_cnt (255) fits MaxFrameNum = 256
    e.set_intra_refresh(True)
    e.close()


def _balancer(fps, npic):
    rows = [tuple(map(int, l.split())) for l in open(os.path.join(ROOT, "tests", "golden", "balancer_adaptive.txt")) if l.strip() and not l.startswith("#")]
    out, k, cur = [], 0, rows[0][1]
    for i in range(npic):
        t = i * 1000.0 / fps
        while k < len(rows) and rows[k][0] <= t:
            cur = rows[k][1]
            k += 1
        out.append(cur)
    return out


def test_cbr_under_the_balancer_script_without_idr_bursts(E):
    """1080p60 CBR driven by the reference's adaptive balancer (tests/golden/balancer_adaptive.txt, picture i at i / 60 s): with intra refresh every
    whole second after the first is within 10 % of its mean setpoint, and the largest access unit after picture 0 is under half the largest IDR
    access unit of the same clip and setpoints with refresh off."""
    w, h, fps, gop, npic = 1920, 1080, 60, 60, 600
    clip = _clip(w, h, 16)
    bps = _balancer(fps, npic)
    res = {}
    for on in (True, False):
        e = E.Encoder(w, h, fps=fps, gop=gop, bitrate_bps=bps[0], pipeline_depth=1, intra_refresh=on, scenecut=False)
        sizes, keys = [], []
        for i in range(npic):
            if i == 0 or bps[i] != bps[i - 1]:
                e.set_bitrate(bps[i])
            y, uv = _pic(clip, i)
            e.submit(y, uv, pts=i)
            if e.pending > 1:
                au, key, _, _ = e.collect(copy=False)
                sizes.append(au); keys.append(key)
        while e.pending:
            au, key, _, _ = e.collect(copy=False)
            sizes.append(au); keys.append(key)
        e.close()
        res[on] = np.array(sizes, float), np.array(keys)
    sizes, _ = res[True]
    for s in range(1, npic // fps):
        rate = sizes[s * fps:(s + 1) * fps].sum() * 8
        want = float(np.mean(bps[s * fps:(s + 1) * fps]))
        assert abs(rate - want) / want < 0.10, (s, rate, want)
    off, key_off = res[False]
    idr_max = off[key_off].max()
    print("largest AU after picture 0: refresh %d bytes, IDR %d bytes" % (sizes[1:].max(), idr_max))
    assert sizes[1:].max() < 0.5 * idr_max, (sizes[1:].max(), idr_max)


def test_a_long_stream_keeps_its_cycle_and_frame_num(E, oracle):
    """More than 512 pictures after the IDR picture: the picture count behind frame_num is kept bounded (modulo 256) and the cycle position is a
    counter of its own -- frame_num still steps by one modulo 256 in every access unit, and the cycles keep their places and decode."""
    w, h, n, npic = 176, 144, 7, 1 + 600
    e = _open(E, w, h, n, depth=2)
    aus, keys, drops, recs = _encode(e, _clip(w, h, 12), npic, 2, fetch=True)
    mbw, mbh = e.mbw, e.mbh
    e.close()
    _check_structure(aus, keys, drops, ["idr"] + ["p"] * (npic - 1), mbw, mbh, n, oracle, recs, 2)
    fns = [_frame_num([b for t, b in _nals(au) if t in (1, 5)][0]) for au in aus]
    assert fns == [i % 256 for i in range(npic)]
