"""Frame-rate conversion on the GPU: the mix launch against tests/rateref.py bit for bit, margins included, and converting streams against
the plain stream of an encoder that is fed the pictures the reference says the ticks show -- byte for byte and pts for pts."""
import ctypes as C

import numpy as np
import pytest

from oracle import csc
from tests import cscref
from tests import overlayref
from tests import rateref as R
from tests import scaleref
from tests.inputref import device_planes
from tests.test_scale_gpu import clip
from tests.util import pad_planes

pytestmark = pytest.mark.gpu

NS = 10 ** 9
QP, GOP, DEPTH = 28, 3, 2
GEOMS = [(208, 120), (200, 112), (16, 16)]  # coded margins in rows, in columns and rows, none
STYLE = dict(xpad=0, ypad=0, scale=1, shaded_background=1)


def _noise(w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h // 2, w), dtype=np.uint8)


# ---- the launch alone
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "%dx%d" % g)
def test_stage_rate_is_bit_exact(E, geom):
    w, h = geom
    e = E.Encoder(w, h, fixed_qp=QP)
    a, b = _noise(w, h, 1), _noise(w, h, 2)
    lo, hi = (np.zeros((h, w), np.uint8), np.zeros((h // 2, w), np.uint8)), (np.full((h, w), 255, np.uint8), np.full((h // 2, w), 255, np.uint8))
    for pa, pb in ((a, b), (lo, hi), (hi, lo)):
        sa, sb = pad_planes(*pa), pad_planes(*pb)
        keep = [p.copy() for p in sa + sb]
        for wt in (0, 1, 43, 128, 171, 255, 256):
            oy, ouv = e.stage_rate(wt, sa[0], sa[1], sb[0], sb[1])
            assert np.array_equal(oy, R.mix(sa[0], sb[0], wt)) and np.array_equal(ouv, R.mix(sa[1], sb[1], wt)), wt
            # the mix of the margins is the replica of the mix
            my, muv = pad_planes(R.mix(pa[0], pb[0], wt), R.mix(pa[1], pb[1], wt))
            assert np.array_equal(oy, my) and np.array_equal(ouv, muv), wt
            if wt in (0, 256):
                assert np.array_equal(oy, (sa if wt == 0 else sb)[0]) and np.array_equal(ouv, (sa if wt == 0 else sb)[1])
        assert all(np.array_equal(k, p) for k, p in zip(keep, sa + sb))  # the caller's a and b are unchanged
    # surfaces whose margins are no replicas are mixed sample for sample all the same
    fa, fb = _noise(e.mbw * 16, e.mbh * 16, 3), _noise(e.mbw * 16, e.mbh * 16, 4)
    oy, ouv = e.stage_rate(85, fa[0], fa[1], fb[0], fb[1])
    assert np.array_equal(oy, R.mix(fa[0], fb[0], 85)) and np.array_equal(ouv, R.mix(fa[1], fb[1], 85))
    with pytest.raises(E.EncoderError):
        e.stage_rate(257, fa[0], fa[1], fb[0], fb[1])
    with pytest.raises(E.EncoderError):
        e.time_stage(E.STAGE_RATE, 1)  # conversion off: there is no mix to time
    e.close()


# ---- streams
def encoder(E, w, h, fps, rate=None, **kw):
    return E.Encoder(w, h, fps=fps, gop=GOP, fixed_qp=QP, pipeline_depth=DEPTH, rate=rate, **kw)


def drive(e, n, need, feed, before=None):
    """n inputs; before input i as many pictures are collected as its submit needs free slots.  -> ([(au, key, pts, qp)], what feed returned per input)"""
    out, ret = [], []
    for i in range(n):
        if before:
            before(i)
        k = need(i)
        while DEPTH + 1 - e.pending < k:
            out.append(e.collect())
        ret.append(feed(i))
    while e.pending:
        out.append(e.collect())
    return out, ret


def convert(e, mode, pts, submit, before=None, idr=()):
    """the converting encoder over inputs at `pts`; checks rate_peek against what each submit then does"""
    peeked = []

    def need(i):
        peeked.append(e.rate_peek(pts[i]))
        return max(peeked[-1], 1 if mode == R.BLEND else 0)
    out, counts = drive(e, len(pts), need, lambda i: submit(i, pts[i], i in idr), before)
    assert counts == peeked
    return out, counts


def expected(E, w, h, fps, mode, pts, sources, max_fill=2, before=None, idr=(), texts=None, **kw):
    """the plain stream of the pictures the reference says the ticks show, submitted in the same groups, with the ticks' pts"""
    steps = R.run(mode, NS, fps, 1, max_fill, pts)
    shown, groups, owed = iter(R.shown(mode, steps)), [], False
    for i, (o, _, _) in enumerate(steps):
        owed |= i in idr
        g = []
        for _ in o:
            t, a, b, wt = next(shown)
            pic = (R.mix(sources[a][0], sources[b][0], wt), R.mix(sources[a][1], sources[b][1], wt))
            if texts:
                pic = overlayref.draw(pic[0], pic[1], texts[i], **STYLE)
            g.append((pic, t, owed))
            owed = False
        groups.append(g)
    e = encoder(E, w, h, fps, **kw)

    def feed(i):
        for pic, t, key in groups[i]:
            e.submit(pic[0], pic[1], pts=t, force_idr=key)
        return len(groups[i])
    out, counts = drive(e, len(pts), lambda i: max(len(groups[i]), 1 if mode == R.BLEND else 0), feed, (lambda i: before(e, i)) if before else None)
    assert e.rate_bytes() == 0
    e.close()
    return out, counts, steps


def same(got, ref):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g == r, (i, len(g[0]), len(r[0]), g[1:], r[1:])


def in_pts(fps_in, n):
    return [i * NS // fps_in for i in range(n)]


@pytest.mark.parametrize("case", [(R.HOLD, 60, 30, 13, (208, 120)), (R.HOLD, 25, 30, 10, (200, 112)), (R.BLEND, 50, 30, 12, (200, 112))],
                         ids=["hold-60-30", "hold-25-30", "blend-50-30"])
def test_stream_from_host_nv12(E, oracle, case):
    mode, fi, fo, n, (w, h) = case
    pics, pts = clip(w, h, n), in_pts(fi, n)
    ref, counts, steps = expected(E, w, h, fo, mode, pts, pics)
    e = encoder(E, w, h, fo, rate=(mode, NS, 2))
    got, got_counts = convert(e, mode, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k))
    st = e.rate_stats()
    dec = oracle.Decoder()
    for g in got:
        dy, duv = dec.decode(g[0])
    assert np.array_equal(dy, e.fetch(E.FETCH_RECON_Y)) and np.array_equal(duv, e.fetch(E.FETCH_RECON_UV))
    assert e.rate_bytes() == e.mbw * e.mbh * 384
    e.close()
    assert got_counts == counts
    same(got, ref)
    ws = [x for _, wl, _ in steps for x in wl]
    assert st == dict({"in": n, "out": len(ref), "dropped": counts.count(0), "resyncs": 0},
                      repeated=sum(c - 1 for c in counts if c) if mode == R.HOLD else 0, blended=sum(0 < x < 256 for x in ws) if mode == R.BLEND else 0)
    assert {R.HOLD: st["dropped"] if fi > fo else st["repeated"], R.BLEND: st["blended"]}[mode] >= 2  # the case does what it is here for


def test_blend_25_to_30_from_yuy2(E):
    w, h, n = 200, 112, 10
    rng = np.random.default_rng(11)
    planes = [cscref.random_planes(E.FMT_YUY2, w, h, rng) for _ in range(n)]
    sources = [tuple(p[:r, :w] for p, r in zip(csc.to_nv12(csc.FMT_YUY2, pl, w, h), (h, h // 2))) for pl in planes]
    pts = in_pts(25, n)
    ref, counts, _ = expected(E, w, h, 30, R.BLEND, pts, sources)
    e = encoder(E, w, h, 30, rate=(R.BLEND, NS, 2))
    got, _ = convert(e, R.BLEND, pts, lambda i, t, k: e.submit_fmt(E.FMT_YUY2, planes[i], pts=t, force_idr=k))
    e.close()
    assert 2 in counts
    same(got, ref)


def test_blend_25_to_30_from_a_scaled_input(E):
    iw, ih, w, h, n = 400, 224, 200, 112, 10
    pics = clip(iw, ih, n)
    sources = [tuple(p[:r, :w] for p, r in zip(scaleref.to_nv12(scaleref.FMT_NV12, [y, uv], iw, ih, w, h), (h, h // 2))) for y, uv in pics]
    pts = in_pts(25, n)
    ref, _, _ = expected(E, w, h, 30, R.BLEND, pts, sources)
    e = encoder(E, w, h, 30, rate=(R.BLEND, NS, 2), input_size=(iw, ih))
    got, _ = convert(e, R.BLEND, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k))
    e.close()
    same(got, ref)


def test_hold_30_to_60_draws_the_new_text_on_the_repeated_picture(E):
    w, h, n = 208, 120, 6
    pics, pts = clip(w, h, n), in_pts(30, n)
    texts = ["  b: %5d rtt: %3d" % (2048 - 100 * i, 40 + i) for i in range(n)]
    ref, counts, _ = expected(E, w, h, 60, R.HOLD, pts, pics, texts=texts)
    assert counts == [1] + [2] * (n - 1)
    e = encoder(E, w, h, 60, rate=(R.HOLD, NS, 2))
    e.set_overlay_style(**STYLE)
    got, _ = convert(e, R.HOLD, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k), before=lambda i: e.set_overlay_text(texts[i]))
    assert e.rate_stats()["repeated"] == n - 1
    e.close()
    same(got, ref)


@pytest.mark.parametrize("mode", [R.HOLD, R.BLEND], ids=["hold", "blend"])
def test_same_rate_in_and_out_is_the_stream_with_conversion_off(E, mode):
    """w = 256 reproduces the input exactly, and the mix launch sits in the input path without a trace in the stream"""
    w, h, n = 200, 112, 6
    pics, pts = clip(w, h, n), in_pts(30, n)
    off = encoder(E, w, h, 30)
    ref, _ = drive(off, n, lambda i: 1, lambda i: off.submit(*pics[i], pts=pts[i]))
    off.close()
    e = encoder(E, w, h, 30, rate=(mode, NS, 2))
    got, counts = convert(e, mode, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k))
    st = e.rate_stats()
    e.close()
    assert counts == [1] * n and (st["dropped"], st["repeated"], st["blended"], st["resyncs"]) == (0, 0, 0, 0)
    same(got, ref)


# ---- state and bookkeeping
def test_too_few_free_slots_leaves_everything_untouched(E):
    """hold 30 -> 60: every input but the first takes two slots.  A submit refused for want of slots has not advanced the plan, the statistics or the stream."""
    w, h, n = 208, 120, 5
    pics, pts = clip(w, h, n), in_pts(30, n)
    ref, _, _ = expected(E, w, h, 60, R.HOLD, pts, pics)
    e = encoder(E, w, h, 60, rate=(R.HOLD, NS, 2))
    out = []
    for i in range(n):
        if e.pending + e.rate_peek(pts[i]) > DEPTH + 1:
            before = (e.rate_stats(), e.pending, e.rate_peek(pts[i]))
            with pytest.raises(E.EncoderError, match="-6"):
                e.submit(*pics[i], pts=pts[i])
            assert (e.rate_stats(), e.pending, e.rate_peek(pts[i])) == before
            while e.pending + e.rate_peek(pts[i]) > DEPTH + 1:
                out.append(e.collect())
        assert e.submit(*pics[i], pts=pts[i]) == (1 if i == 0 else 2)
    while e.pending:
        out.append(e.collect())
    e.close()
    same(out, ref)


def test_a_dropped_submits_force_idr_lands_on_the_next_picture(E):
    w, h, n = 208, 120, 7
    pics, pts = clip(w, h, n), in_pts(60, n)
    ref, counts, _ = expected(E, w, h, 30, R.HOLD, pts, pics, idr=(1, 4))  # input 1 is dropped, input 4 too: pictures 1 and 3 are forced
    assert counts == [1, 0, 1, 1, 0, 0, 1] and [r[1] for r in ref] == [True, True, False, True]
    e = encoder(E, w, h, 30, rate=(R.HOLD, NS, 2))
    got, _ = convert(e, R.HOLD, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k), idr=(1, 4))
    e.close()
    same(got, ref)


def test_memory_encode_and_resync(E):
    w, h = 208, 120
    pics = clip(w, h, 4)
    e = E.Encoder(w, h, fps=30, fixed_qp=QP)  # conversion off
    assert e.rate_bytes() == 0 and e.rate_peek(5) == 1 and e.submit(*pics[0], pts=0) is None
    with pytest.raises(E.EncoderError, match="-6"):
        e.rate_stats()
    e.collect()
    assert e.L.mi355enc_set_rate_conversion(e.h, C.byref(E.Rate(1, NS, 0))) == E.ERR_STATE  # after the first submit
    e.close()
    e = E.Encoder(w, h, fps=30, fixed_qp=QP, rate=(R.HOLD, NS, 2))  # pipeline_depth 0 clamps max_fill to 0: nothing is ever repeated, nothing is kept
    assert e.rate_bytes() == 0
    with pytest.raises(E.EncoderError, match="-6"):
        e.encode(*pics[0], pts=0)
    got = []
    for i, t in enumerate([0, NS // 30, NS, NS + NS // 30]):  # a hole of a second: a resync, not 28 repeats
        assert e.rate_peek(t) == 1 and e.submit(*pics[i], pts=t) == 1
        got.append(e.collect()[2])
    assert got == [0, NS // 30, NS, NS + NS // 30] and e.rate_stats()["resyncs"] == 1
    e.close()
    e = E.Encoder(w, h, fps=30, fixed_qp=QP, rate=(R.BLEND, 90000, 0))
    assert e.rate_bytes() == e.mbw * e.mbh * 384
    e.close()
    with pytest.raises(E.EncoderError, match="-1"):
        E.Encoder(w, h, fps=30, rate=(3, NS, 0))


def test_submit_device_leaves_the_callers_planes(E):
    """aligned planes at a stride of 16 n: without conversion the kernels read them in place; with it they are copied, mixed in the copy and never written"""
    w, h, n = 208, 112, 8
    pics, pts = clip(w, h, n), in_pts(25, n)
    ref, _, _ = expected(E, w, h, 30, R.BLEND, pts, pics)
    dev = [device_planes(E, [y, uv], [h, h // 2], [w, w], w, 0) for y, uv in pics]
    e = encoder(E, w, h, 30, rate=(R.BLEND, NS, 2))
    got, _ = convert(e, R.BLEND, pts, lambda i, t, k: e.submit_device(dev[i][2][0], w, dev[i][2][1], w, pts=t, force_idr=k))
    e.close()
    for (hip, buf, _), (y, uv) in zip(dev, pics):
        back = np.empty(w * h * 3 // 2, np.uint8)
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, C.c_size_t(back.size), 2) == 0  # hipMemcpyDeviceToHost
        assert np.array_equal(back[:w * h].reshape(h, w), y) and np.array_equal(back[w * h:].reshape(h // 2, w), uv)
        hip.hipFree(buf)
    same(got, ref)


def test_off_is_off(E):
    w, h, n = 208, 120, 5
    pics = clip(w, h, n)
    streams = []
    for rate in (None, (R.OFF, NS, 2)):
        e = encoder(E, w, h, 30, rate=rate)
        out, _ = drive(e, n, lambda i: 1, lambda i: e.submit(*pics[i], pts=i))
        assert (e.rate_bytes(), e.image_bytes(), e.snapshot_bytes(), e.orient_bytes()) == (0, 0, 0, 0)
        with pytest.raises(E.EncoderError, match="-6"):
            e.rate_stats()
        e.close()
        streams.append(out)
    same(streams[1], streams[0])


def test_recovery_does_not_mix_twice(E):
    """Blend 25 -> 30, three pictures in flight when the tripped word is seen: the pictures come back through recover(), which enqueues their surfaces again --
    with the mix already in them, and without touching the kept input.  The plain encoder goes through the same trip."""
    w, h, n = 208, 120, 9
    pics, pts = clip(w, h, n), in_pts(25, n)
    ref, counts, steps = expected(E, w, h, 30, R.BLEND, pts, pics, before=lambda e, i: e.debug_trip_wait(12) if i == 4 else None)
    assert any(0 < x < 256 for x in steps[4][1])  # the picture submitted right behind the trip is a blended one
    e = encoder(E, w, h, 30, rate=(R.BLEND, NS, 2))
    got, _ = convert(e, R.BLEND, pts, lambda i, t, k: e.submit(*pics[i], pts=t, force_idr=k), before=lambda i: e.debug_trip_wait(12) if i == 4 else None)
    st = e.stats()
    e.close()
    assert st.recoveries == 1
    same(got, ref)


def test_time_stage_runs_the_mix_launch(E):
    e = E.Encoder(208, 120, fps=30, fixed_qp=QP, pipeline_depth=1, rate=(R.BLEND, NS, 1))
    assert 0 < e.time_stage(E.STAGE_RATE, 3) < 50
    e.close()
